"""The Python front end (causalgpslc.jl_amd/api.py) characterised without a GPU and without the library: for every combination
of level kind and keywords that the estimation entry points accept, and for the malformed inputs that have an order of their
own, EITHER the exception (type, full message, and how many library calls were made before it: 0 for every refusal) OR the exact
sequence of C calls — symbol, every scalar by value, NULL as null, every `const` array as shape / strides / SHA-256 of its bytes,
every output array as shape / strides — plus the shapes, strides and bytes of what the public function returns.

Seam: `_lib.load()` hands out the object cached in `_lib._lib`; while a case runs that object is a recorder whose every
`gpslc_*` attribute notes its arguments and returns status 0 (the real one is put back afterwards).  The `c_void_p` that `api._p`
makes with `ndarray.ctypes.data_as` carries its array as `._arr`, so the recorder sees the array behind every pointer.  Parameter
names come from the header (`header_param_names` of test_julia_binding.py); a `double*` parameter without `const` is an output.
Outputs are `np.empty` in the front end: the recorder fills each with a pattern of its index, so what is computed from them (the
group axis squeezed, ITEsamples' and sampleEffectCurve's reorderings, the arrays handed on to gpslc_sate_samples /
gpslc_curve_samples) is deterministic and is pinned as well.

tests/golden/frontend_dispatch.json was written by this module's `__main__` from the api.py of the commit named under "parent"
(a tree of that commit without any built library), recorded twice with equal results:

    python tests/test_frontend_dispatch.py --tree DIR_WITH_THE_PARENT_TREE --parent HASH

Argument descriptions and whole records repeat a lot, so the file stores each distinct one once ("values", "records") and the
cases as indices; `_expand` turns a stored record back into the named form the comparison (and its failure message) uses."""
import contextlib
import ctypes as C
import functools
import hashlib
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cases  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "frontend_dispatch.json")

# ---- the grid ----------------------------------------------------------------------------------------------------------
CASE = cases.make_case(12, "UX", False, S=2, seed=1)
N, S, T = 12, 2, CASE["T"]
W1 = (np.arange(N) + 1.0) / np.sum(np.arange(N) + 1.0)
W2 = np.stack([W1, W1[::-1]])
LEVELS = {"many": {"s": [0.6, 0.2], "v": np.stack([T + 0.5, T])}, "one": {"s": 0.6, "v": T + 0.5}}
KEYWORDS = {"baseline": {"": None, "b": 0.1}, "weights": {"": None, "w1": W1, "w2": W2}, "slope": {"": False, "s": True},
            "outcome": {"": False, "o": True}, "devices": {"": None, "d": [0, 0]}}
ALL5 = ("baseline", "weights", "slope", "outcome", "devices")
# name -> (function, kind of levels, positional arguments after the levels, fixed keywords, the keywords it accepts)
FUNCTIONS = {
    "predict": ("predict", "many", (), {}, ALL5),
    "predict+draws": ("predict", "many", (), dict(want_mean_ite=True, spp=2, want_draws=True), ALL5),
    "SATEDistributions": ("SATEDistributions", "one", (), {}, ALL5[:4]),
    "ITEDistributions": ("ITEDistributions", "one", (), {}, ("baseline", "slope", "outcome")),
    "ITEsamples": ("ITEsamples", "one", (2,), {}, ("baseline", "slope", "outcome")),
    "sampleITE": ("sampleITE", "one", (), dict(samplesPerPosterior=2), ("baseline", "slope", "outcome")),
    "sampleSATE": ("sampleSATE", "one", (), dict(samplesPerPosterior=2), ALL5[:4]),
    "effectCurve": ("effectCurve", "many", (), {}, ALL5),
    "sampleEffectCurve": ("sampleEffectCurve", "many", (), dict(samplesPerPosterior=2), ALL5),
    "_predict_curve": ("_predict_curve", "many", (), dict(want_cov=False), ALL5),
    "_predict_curve+cov": ("_predict_curve", "many", (), dict(want_cov=True), ALL5),
    "predictCounterfactualEffects": ("predictCounterfactualEffects", None, (2,), dict(fidelity=3), ("devices", "outcome")),
}


def _ramp(*shape):
    return np.arange(np.prod(shape), dtype=np.float64).reshape(shape) / np.prod(shape)


def _grid():
    out = {}
    for name, (fn, kind, pos, fixed, accepted) in FUNCTIONS.items():
        for lv in (LEVELS[kind] if kind else {"-": None}):
            for labels in itertools.product(*[KEYWORDS[k] for k in accepted]):
                kw = dict(fixed, **{k: KEYWORDS[k][lab] for k, lab in zip(accepted, labels)})
                args = pos if kind is None else (LEVELS[kind][lv],) + pos
                out[f"{name}|{lv}|{'.'.join(x for x in labels if x)}"] = (fn, args, kw)
    for lv, doT in LEVELS["one"].items():
        p = [None if CASE[k] is None else CASE[k][..., 0] for k in ("uyLS", "xyLS", "tyLS", "yNoise", "yScale", "U")]
        out[f"conditionalITE|{lv}|"] = ("conditionalITE", (*p, CASE["X"], CASE["T"], CASE["Y"], doT), {})
    # malformed inputs, and well-formed ones that take a path of their own; each also with outcome=True, baseline=0.0 on top
    # (where the function has the keyword and the case does not set it), and each with slope=True, which pins the precedence
    # between the keyword refusals and the shape errors
    bad = {
        "doTs-3d": ((np.zeros((2, 2, N)),), {}),
        "doTs-n+1": ((np.zeros((2, N + 1)),), {}),
        "baseline-len": (([0.6, 0.2],), dict(baseline=[0.1, 0.2, 0.3])),
        "baseline-len+weights-len": (([0.6, 0.2],), dict(baseline=[0.1, 0.2, 0.3], weights=np.ones(N + 1))),
        "weights-row-len": (([0.6, 0.2],), dict(weights=[W1, W1[:5]])),
        "weights-empty-mask": (([0.6, 0.2],), dict(weights=np.zeros(N, dtype=bool))),
        "weights-nonfinite": (([0.6, 0.2],), dict(weights=np.where(np.arange(N) == 3, np.nan, W1))),
        "weights-3d": (([0.6, 0.2],), dict(weights=np.ones((1, 2, N)))),
        "weights-mask-row": (([0.6, 0.2],), dict(weights=[T > np.median(T), W1])),
        "z": (([0.6, 0.2],), dict(spp=2, want_draws=True, z=_ramp(N, 2, S, 2))),
        "z-shape": (([0.6, 0.2],), dict(spp=2, want_draws=True, z=_ramp(N, 1, S, 2))),
        "z-shape+devices": (([0.6, 0.2],), dict(spp=2, want_draws=True, z=_ramp(N, 1, S, 2), devices=[0, 0])),
    }
    extra = {f"{name}|{k}": (name, a, kw) for name in ("predict", "_predict_curve") for k, (a, kw) in bad.items()}
    extra.update({
        "ITEDistributions|baseline-len": ("ITEDistributions", (0.6,), dict(baseline=[0.1, 0.2])),
        "ITEDistributions|doT-n+1": ("ITEDistributions", (np.zeros(N + 1),), {}),
        "ITEDistributions|doT-2d": ("ITEDistributions", (np.zeros((1, N)),), {}),
        "SATEDistributions|doT-n+1": ("SATEDistributions", (np.zeros(N + 1),), {}),
        "SATEDistributions|doT-n+1+weights-len": ("SATEDistributions", (np.zeros(N + 1),), dict(weights=np.ones(N + 1))),
        "sampleSATE|w2+z": ("sampleSATE", (0.6,), dict(samplesPerPosterior=2, weights=W2, z=_ramp(2, S * 2))),
        "sampleSATE|w2+z-shared": ("sampleSATE", (0.6,), dict(samplesPerPosterior=2, weights=W2, z=_ramp(S * 2))),
        "ITEsamples|z": ("ITEsamples", (0.6, 2), dict(z=_ramp(N, S * 2))),
        "sampleEffectCurve|w1+z": ("sampleEffectCurve", ([0.6, 0.2],), dict(samplesPerPosterior=2, weights=W1, z=_ramp(2, 2, S))),
        "sampleEffectCurve|w2+z": ("sampleEffectCurve", ([0.6, 0.2],), dict(samplesPerPosterior=2, weights=W2, z=_ramp(2, 2, S, 2))),
        "predictCounterfactualEffects|z": ("predictCounterfactualEffects", (2,), dict(fidelity=3, z=_ramp(4, N, S * 2))),
        "predictCounterfactualEffects|empty-range": ("predictCounterfactualEffects", (2,), dict(minDoT=1.0, maxDoT=0.0)),
    })
    for cid, (fn, args, kw) in extra.items():
        out[cid] = (fn, args, kw)
        on_top = {k: v for k, v in (("baseline", 0.0), ("outcome", True)) if k in FUNCTIONS[fn][4]}
        out[cid + "|" + ".".join(k[0] for k in on_top)] = (fn, args, dict(on_top, **kw))
        if "slope" in FUNCTIONS[fn][4]:
            out[cid + "|s"] = (fn, args, dict(kw, slope=True))
    return out


CASES = _grid()
# 681 refusals (629 + 47 + 5 of z's shape), 151 cases that reach the library; the 19 symbols are gpslc_create, gpslc_set_data, the nine
# gpslc_predict*, the six gpslc_ite_distributions*, gpslc_sate_samples and gpslc_curve_samples
EXPECTED_COUNTS = {"cases": 832, "ValueError": 629, "NotImplementedError": 47, "AssertionError": 5, "reach": 151, "symbols": 19}


# ---- the recorder ------------------------------------------------------------------------------------------------------
def _array(a, with_bytes=True):
    # the stride of an axis of length 1, and every stride of an empty array, addresses nothing and varies with NumPy's version
    strides = [st if ln > 1 and a.size else 0 for ln, st in zip(a.shape, a.strides)]
    d = f"{a.dtype.str[1:]}{list(a.shape)}/{strides}"
    return d + "#" + hashlib.sha256(a.tobytes()).hexdigest()[:12] if with_bytes else d


@functools.lru_cache(maxsize=None)
def _header():
    """symbol -> [(parameter name, is an output array)]"""
    from causalgpslc_jl_amd import _lib
    from test_julia_binding import header_param_names
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    out = {}
    for sym, names in header_param_names().items():
        decls = re.search(r"\b" + sym + r"\s*\(([^)]*)\)\s*;", txt).group(1).split(",")
        out[sym] = [(nm, bool(re.match(r"\s*double\s*\*", d))) for nm, d in zip(names, decls)]
    return out


class Recorder:
    def __init__(self, header):
        self.header, self.calls = header, []

    def __getattr__(self, sym):
        if not sym.startswith("gpslc_"):
            raise AttributeError(sym)

        def call(*args):
            params = self.header[sym]
            assert len(args) == len(params), (sym, len(args), len(params))
            entry = {}
            for (name, is_out), v in zip(params, args):
                arr = getattr(v, "_arr", None)
                if v is None or isinstance(v, (bool, int, float)):
                    entry[name] = v
                elif isinstance(arr, np.ndarray):
                    entry[name] = _array(arr, with_bytes=not is_out)
                    if is_out:
                        arr[...] = 1.0 + 0.5 * np.arange(arr.size, dtype=np.float64).reshape(arr.shape)
                elif isinstance(v, C.Array):
                    entry[name] = f"{type(v)._type_.__name__}[{len(v)}]"
                else:
                    entry[name] = type(v).__name__           # a context handle, byref(handle)
            self.calls.append([sym, entry])
            return 0
        return call


@contextlib.contextmanager
def recording(gp):
    lib, saved = Recorder(_header()), gp._lib._lib
    gp._lib._lib = lib
    try:
        yield lib
    finally:
        gp._lib._lib = saved


def _returned(r):
    if isinstance(r, np.ndarray):
        return _array(r)
    if isinstance(r, (tuple, list)):
        return [_returned(x) for x in r]
    return r if r is None or isinstance(r, (bool, int, float)) else type(r).__name__


def run(gp, case_id):
    name, args, kw = CASES[case_id]
    fn = getattr(gp.api, name)
    with recording(gp) as lib:
        if name != "conditionalITE":
            args = (cases.gpslc_object(gp, CASE),) + tuple(args)
        try:
            rec = {"returns": _returned(fn(*args, **kw)), "calls": lib.calls}
        except Exception as e:
            rec = {"raises": [type(e).__name__, str(e), len(lib.calls)]}
    return json.loads(json.dumps(rec))


def _expand(fx, idx):
    rec = dict(fx["records"][idx])
    if "calls" in rec:
        hdr = _header()
        rec["calls"] = [[sym, {nm: fx["values"][i] for (nm, _), i in zip(hdr[sym], ids)}] for sym, *ids in rec["calls"]]
        rec["returns"] = fx["values"][rec["returns"]]
    return rec


def _counts(records):
    """What the fixture holds, in a few numbers: cases, refusals by exception type, cases that reach the library, and the
    distinct symbols those reach (gpslc_create / gpslc_set_data included)."""
    out = {"cases": len(records), "reach": 0}
    syms = set()
    for rec in records:
        if "raises" in rec:
            out[rec["raises"][0]] = out.get(rec["raises"][0], 0) + 1
        else:
            out["reach"] += 1
            syms.update(c[0] for c in rec["calls"])
    out["symbols"] = len(syms)
    return out


# ---- the tests ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def front_end():
    import causalgpslc_jl_amd as gp_
    return gp_


def test_every_case_was_recorded_and_no_other(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert len(recorded["parent"]) == 40 and recorded["repeatable"] is True
    counts = _counts([_expand(recorded, i) for i in recorded["cases"].values()])
    assert counts == recorded["counts"]
    assert counts == EXPECTED_COUNTS
    # every refusal comes before any library call, the context's creation included; only z's shape is checked after it
    for cid, i in recorded["cases"].items():
        r = recorded["records"][i].get("raises")
        if r is not None and r[2] != 0:
            assert r[0] == "AssertionError" and r[1].startswith("z must be"), cid


@pytest.mark.parametrize("case_id", list(CASES))
def test_the_front_end_does_what_the_parent_did(front_end, recorded, case_id):
    assert run(front_end, case_id) == _expand(recorded, recorded["cases"][case_id]), case_id


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", required=True, help="a tree of the parent commit (causalgpslc_jl_amd.py, the package, include/)")
    ap.add_argument("--parent", required=True, help="that commit's 40-character hash")
    a = ap.parse_args()
    assert len(a.parent) == 40
    sys.path.insert(0, os.path.abspath(a.tree))
    import causalgpslc_jl_amd as gp
    assert os.path.abspath(gp.api.__file__).startswith(os.path.abspath(a.tree) + os.sep), gp.api.__file__
    first = {cid: run(gp, cid) for cid in CASES}
    assert first == {cid: run(gp, cid) for cid in CASES}, "the two recordings differ"
    values, records, table = [], [], {}

    def intern(store, v):
        key = (id(store), json.dumps(v, sort_keys=True))
        if key not in table:
            table[key] = len(store)
            store.append(v)
        return table[key]

    fx = {"parent": a.parent, "repeatable": True, "counts": _counts(list(first.values())), "cases": {}}
    for cid, rec in first.items():
        if "calls" in rec:
            rec = {"calls": [[sym] + [intern(values, v) for v in entry.values()] for sym, entry in rec["calls"]],
                   "returns": intern(values, rec["returns"])}
        fx["cases"][cid] = intern(records, rec)
    fx["values"], fx["records"] = values, records
    with open(FIXTURE, "w") as f:
        json.dump(fx, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(json.dumps(fx["counts"], sort_keys=True), len(records), "records,", len(values), "values,", os.path.getsize(FIXTURE), "bytes")
