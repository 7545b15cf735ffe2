"""Host-side mirror of the reference's interface for the hot path.

Names, argument meaning and error behaviour follow CausalGPSLC.jl so that the parity tests read
like the reference's own tests:

    rbfKernelLog, processCov                      src/kernel.jl:24-32, 53-59
    GPSLCObject (data + flattened posterior)      src/types.jl:249-258, src/utils.jl:92-124
    conditionalITE, ITEDistributions, ITEsamples,
    conditionalSATE, SATEDistributions, SATEsamples   src/estimation.jl:36-163
    sampleITE, sampleSATE, summarizeEstimates     src/driver.jl:86-89, 108-111, 129-149
    predictCounterfactualEffects                  src/prediction.jl:23-36
    yLogpdf                                       src/model_likelihood.jl:83-120 (:Y node score)
    looPredictive, looSummary                     leave-one-out checks of that node's outcome model (no reference counterpart)
    yLogpdfGrad                                   gradient of that node's score in U, the hyper-parameters and Y (no reference counterpart)
    lgoPredictive, lgoSummary, foldLabels         leave-group-out checks of it, groups of at most 128 members (no reference counterpart)
    kfoldPredictive, kfoldSummary                 K-fold cross-validation of it: groups of any size (no reference counterpart)
    predictNew                                    outcome, contrast or slope at individuals who are not in the data (no reference counterpart)
    averageNew                                    their weighted averages over a target population, with variance and joint covariance (no reference counterpart)

Everything numeric is done by libgpslc_hip.so through the C ABI (``_lib``); this module only
marshals arrays (NumPy, column-major) and reproduces the reference's output layouts.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import GPSLCError, PosDefException

PREDICTION_COVARIANCE_NOISE = 1e-10   # src/hyperparameters.jl:92


def _f(a, shape=None):
    """float64, column-major, contiguous."""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.astype(np.float64)
    a = np.asfortranarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise AssertionError(f"expected shape {shape}, got {a.shape}")
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _intervention(doT, n):
    """An ``Intervention`` (src/types.jl:138-143) for n individuals -> (scalar, None) or (None, d).

    A Python / NumPy scalar or Bool is one level for everyone (``fill(doT, n)``); a 1-D array or list of length n (Bool ->
    0/1) gives each individual its own treatment value.  Any other shape raises ValueError before anything runs on a device."""
    a = np.asarray(doT)
    if a.ndim == 0:
        return float(a), None
    if a.ndim == 1 and a.shape[0] == n:
        return None, np.ascontiguousarray(a, dtype=np.float64)
    raise ValueError(f"doT must be a scalar or a vector of length n = {n}, got an array of shape {a.shape}")


def _baseline(baseline, L):
    """The ``baseline=`` of a contrast (gpslc_predict_contrast) for L scalar levels -> (L,) float64: a scalar (Bool -> 0/1)
    is every level's baseline, a 1-D sequence gives each level its own.  Any other shape raises ValueError before anything
    runs on a device."""
    b = np.asarray(baseline, dtype=np.float64)
    if b.ndim == 0:
        return np.full(L, float(b))
    if b.ndim == 1 and b.shape[0] == L:
        return np.ascontiguousarray(b)
    raise ValueError(f"baseline must be a scalar or one value per level (L = {L}), got an array of shape {b.shape}")


def _weight_row(w, n):
    """One weight vector for n individuals -> (n,) float64.  Float (or integer) values are used as given; a Bool vector is a
    group mask and becomes that group's average, ``mask / mask.sum()`` (an empty mask raises ValueError)."""
    a = np.asarray(w)
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError(f"weights must be a vector of length n = {n} or a (G, n) array, got a row of shape {a.shape}")
    if a.dtype == np.bool_:
        k = int(a.sum())
        if k == 0:
            raise ValueError("weights has an empty group mask: the average over nobody is undefined")
        return a.astype(np.float64) / k
    a = a.astype(np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("weights has a non-finite entry")
    return a


def _weights(weights, n):
    """The ``weights=`` of predict / SATEDistributions / sampleSATE -> ((G, n) float64 C-contiguous, is_vector): a length-n
    vector (one weight column, results without a group axis) or a (G, n) array / a sequence of G rows, each row parsed by
    ``_weight_row`` (Float rows as given, Bool rows as group masks).  Raises ValueError before anything runs on a device."""
    if isinstance(weights, (list, tuple)) and len(weights) > 0 and np.ndim(weights[0]) == 1:
        return np.ascontiguousarray(np.stack([_weight_row(r, n) for r in weights])), False
    a = np.asarray(weights)
    if a.ndim == 1:
        return np.ascontiguousarray(_weight_row(a, n)[None, :]), True
    if a.ndim == 2 and a.shape[0] >= 1 and a.shape[1] == n:
        return np.ascontiguousarray(np.stack([_weight_row(r, n) for r in a])), False
    raise ValueError(f"weights must be a vector of length n = {n} or a (G, n) array, got an array of shape {a.shape}")


def groupWeights(labels):
    """Group-average weights for a labelling of the n individuals (object labels of the hierarchy, strata, a treatment
    indicator): returns (the sorted distinct labels (G,), W (G, n)) with W[g] = 1_{labels == label_g} / |group g| — the
    ``weights=`` of predict / SATEDistributions / sampleSATE.  The groups partition the sample, so
    sum_g (n_g / n) * mean_g is the meanSATE of the plain call."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] == 0:
        raise ValueError(f"labels must be a non-empty vector (one label per individual), got an array of shape {lab.shape}")
    keys, inv = np.unique(lab, return_inverse=True)
    W = np.zeros((keys.shape[0], lab.shape[0]))
    W[inv, np.arange(lab.shape[0])] = 1.0
    W /= W.sum(axis=1, keepdims=True)
    return keys, W


# What a level call cannot ask for, refused before any device work: (condition on the request, exception, message).  The first
# row that fires is the call's complaint.  ``q.caller`` is "predict", "curve" (_predict_curve) or "distributions"
# (_ite_distributions); ``q.vec``: per-individual levels; ``q.base`` / ``q.w`` / ``q.dev``: baseline= / weights= / devices= given.
_REFUSALS = (
    (lambda q: q.outcome and q.base, ValueError,
     "outcome=True cannot be combined with baseline=: the contrast is the difference of two outcomes, "
     "f(a) - f(b); ask for the contrast, or for the outcomes at a and at b"),
    (lambda q: q.outcome and q.slope, ValueError,
     "outcome=True cannot be combined with slope=True: the outcome is a level of the surface, the slope its derivative"),
    (lambda q: q.outcome and q.dev, ValueError, "outcome=True is not sharded over devices: call without devices="),
    (lambda q: q.outcome and q.w and q.vec and q.caller == "predict", ValueError,
     "outcome=True with weights= needs scalar levels: weighted outcomes at per-individual intervention "
     "vectors are not supported"),
    (lambda q: q.slope and q.base, ValueError,
     "slope=True cannot be combined with baseline=: the slope is a derivative at one level, not a contrast"),
    (lambda q: q.slope and q.vec, ValueError,
     "slope=True needs scalar levels: slopes at per-individual intervention vectors are not supported"),
    (lambda q: q.slope and q.dev, ValueError, "slope=True is not sharded over devices: call without devices="),
    (lambda q: q.caller == "curve" and q.vec, ValueError,
     "an effect curve needs scalar levels: per-individual intervention vectors are not supported"),
    (lambda q: q.caller == "curve" and q.dev, NotImplementedError,
     "effect curves are not sharded over devices: call without devices="),
    (lambda q: len(q.shape) > 2 or (q.vec and q.shape[1] != q.n), ValueError,
     "doTs must be L scalar levels or an (L, n) array of intervention vectors with n = {n}, got an array of shape {shape}"),
    (lambda q: q.vec and q.dev, NotImplementedError,
     "vector interventions are not sharded over devices: call predict without devices="),
    (lambda q: q.base and q.vec and q.caller == "predict", ValueError,
     "baseline= needs scalar levels: contrasts of per-individual intervention vectors are not supported"),
    (lambda q: q.base and q.vec and q.caller == "distributions", ValueError,
     "baseline= needs a scalar doT: contrasts of per-individual intervention vectors are not supported"),
    (lambda q: q.base and q.dev, NotImplementedError, "contrasts are not sharded over devices: call predict without devices="),
    (lambda q: q.w and q.vec, ValueError,
     "weights= needs scalar levels: weighted effects of per-individual intervention vectors are not supported"),
    (lambda q: q.w and q.dev, NotImplementedError, "weighted effects are not sharded over devices: call predict without devices="),
)


def _refuse(caller, shape=(0,), n=0, baseline=None, weights=None, slope=False, outcome=False, devices=None):
    """Raise the first row of ``_REFUSALS`` that the request (levels of this shape for n individuals, these keywords) meets.
    Vector levels are a 2-D array; a curve takes every array beyond 1-D for them, where predict complains of its shape."""
    q = SimpleNamespace(caller=caller, shape=shape, n=n, vec=len(shape) == 2 or (caller == "curve" and len(shape) > 2),
                        base=baseline is not None, w=weights is not None, slope=slope, outcome=outcome, dev=devices is not None)
    for cond, exc, msg in _REFUSALS:
        if cond(q):
            raise exc(msg.format(n=n, shape=shape))


@dataclass(frozen=True)
class _Plan:
    """One level call, normalised: what ``predict``, ``_predict_curve`` and ``_ite_distributions`` hand to ``_SYMBOLS``."""
    caller: str                    # "predict", "curve" or "distributions"
    form: str                      # as csrc/level_form.h names it: "ordinary", "contrast", "slope" or "outcome"
    vec: bool                      # per-individual levels
    levels: np.ndarray             # (L,), or (n, L) column-major for vector levels: doT[i + n*l]
    base: Optional[np.ndarray]     # (L,) for a contrast
    W: Optional[np.ndarray]        # (G, n) C order = weights[i + n*g]
    wvec: bool                     # ``weights`` was one vector: the caller drops the group axis
    devices: Optional[Sequence[int]]

    L = property(lambda self: self.levels.shape[-1])
    weighted = property(lambda self: self.W is not None)
    sharded = property(lambda self: self.devices is not None)


def _plan(g, doTs, caller, baseline=None, weights=None, slope=False, outcome=False, devices=None) -> _Plan:
    """Refuse (``_REFUSALS``, then the parse errors of ``_weights`` and ``_baseline``) or describe the call.  Nothing here
    touches a device.  A curve's ``weights=None`` is 1/n for everybody."""
    n = g.getN()
    a = np.asarray(doTs, dtype=np.float64)
    _refuse(caller, a.shape, n, baseline, weights, slope, outcome, devices)
    W, wvec = (None, False) if weights is None else _weights(weights, n)
    if W is None and caller == "curve":
        W, wvec = np.full((1, n), 1.0 / n), True
    vec = a.ndim == 2
    levels = np.asfortranarray(a.T) if vec else np.ascontiguousarray(np.atleast_1d(a))
    base = None if baseline is None else _baseline(baseline, levels.shape[-1])
    form = "outcome" if outcome else "slope" if slope else "ordinary" if base is None else "contrast"
    return _Plan(caller, form, vec, levels, base, W, wvec, devices)


# The entry points of the C boundary that take levels: (symbol, the plan fields that select it, the optional arguments it has
# besides the common ones).  The first row whose every field equals the plan's is the call's.  "base": doT_base (NULL for no
# contrast); "weights": G, weights (0, NULL for none); "cov": covW; "multi": nctx, ctxs in place of ctx and a trailing info.
_SYMBOLS = (
    ("gpslc_ite_distributions_outcome_vec", dict(caller="distributions", form="outcome", vec=True), ()),
    ("gpslc_ite_distributions_outcome", dict(caller="distributions", form="outcome"), ()),
    ("gpslc_ite_distributions_slope", dict(caller="distributions", form="slope"), ()),
    ("gpslc_ite_distributions_contrast", dict(caller="distributions", form="contrast"), ("base",)),
    ("gpslc_ite_distributions_vec", dict(caller="distributions", vec=True), ()),
    ("gpslc_ite_distributions", dict(caller="distributions"), ()),
    ("gpslc_predict_outcome_vec", dict(form="outcome", vec=True), ()),
    ("gpslc_predict_outcome", dict(form="outcome"), ("weights", "cov")),
    ("gpslc_predict_slope", dict(form="slope"), ("weights", "cov")),
    ("gpslc_predict_curve", dict(caller="curve"), ("base", "weights", "cov")),
    ("gpslc_predict_weighted", dict(weighted=True), ("base", "weights")),
    ("gpslc_predict_contrast", dict(form="contrast"), ("base",)),
    ("gpslc_predict_vec", dict(vec=True), ()),
    ("gpslc_predict_multi", dict(sharded=True), ("multi",)),
    ("gpslc_predict", dict(), ()),
)


def _symbol(p: _Plan):
    return next((sym, opt) for sym, sel, opt in _SYMBOLS if all(getattr(p, k) == v for k, v in sel.items()))


NEW_FORMS = {"outcome": 0, "contrast": 1, "slope": 2}      # GPSLC_NEW_* of the header


class Context:
    """RAII wrapper of gpslc_ctx (one per GPU and data set)."""

    def __init__(self, n, nX, nU, device=0, profile=False, fp32_kernel=False):
        self.lib = _lib.load()
        self.n, self.nX, self.nU = int(n), int(nX), int(nU)
        h = C.c_void_p()
        st = self.lib.gpslc_create(C.byref(h), int(device), self.n, self.nX, self.nU,
                                   (1 if profile else 0) | (2 if fp32_kernel else 0))
        if st != 0:
            raise GPSLCError(st, {-1003: "no usable gfx950 device"}.get(st, "gpslc_create failed"))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpslc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st):
        if st < 0:
            raise GPSLCError(st, self.lib.gpslc_last_error(self.h).decode())
        if st > 0:
            raise PosDefException(st)

    def set_data(self, X, T, Y):
        X = None if self.nX == 0 else _f(X).reshape(self.n, self.nX, order="F")
        T = _f(T, (self.n,))
        Y = _f(Y, (self.n,))
        self._keep = (X, T, Y)
        self.check(self.lib.gpslc_set_data(self.h, _p(X), _p(T), _p(Y)))

    def set_tuning(self, max_batch=0, panel_tiles=0, n_streams=0):
        self.check(self.lib.gpslc_set_tuning(self.h, max_batch, panel_tiles, n_streams))

    def set_task_schedule(self, min_tiles=0, max_tiles=-1, min_matrices=0, group=0):
        """Persistent factorisation launch for chunks of at least min_matrices matrices of min_tiles .. max_tiles tiles per
        side (max_tiles = 0: off; 0 / -1 / 0 / 0 = keep)."""
        self.check(self.lib.gpslc_set_task_schedule(self.h, min_tiles, max_tiles, min_matrices, group))

    def set_ensemble(self, sample_offset=0, S_total=0):
        """Placement of the next calls' samples inside a larger ensemble (Philox stream ids): gpslc_set_ensemble."""
        self.check(self.lib.gpslc_set_ensemble(self.h, int(sample_offset), int(S_total)))

    def last_info(self, S):
        out = np.zeros(S, dtype=np.int32)
        self.check(self.lib.gpslc_last_info(self.h, out.ctypes.data_as(_lib.c_int32_p), S))
        return out

    def _call_for(self, fn, shapes, want, *args, fill=np.nan):
        """What y_loo, y_lgo, y_logpdf_grad and predict_new share: one column-major array per output named in ``want`` (``shapes``:
        every output's shape, in the order of ``fn``'s trailing pointer arguments) full of ``fill`` (None: as allocated), None
        (NULL to the library) for the others -> ``(status, outputs)``.  ``args`` go before them: host arrays as given (None =
        NULL), numbers and ctypes pointers as they are."""
        out = {k: (np.empty(s, order="F") if fill is None else np.full(s, fill, order="F")) if k in want else None
               for k, s in shapes.items()}
        return fn(self.h, *[_p(a) if isinstance(a, np.ndarray) else a for a in args], *map(_p, out.values())), out

    def y_loo(self, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, want=("mean", "var", "lpd", "logpdf")):
        """gpslc_y_loo with host arrays as given (None = NULL): ``(status, looMean, looVar, looLpd, logpdf)`` — the outputs
        named in ``want`` as (n, S) / (S,) arrays, the others None (NULL to the library).  The status is returned, not raised:
        a positive one (a parameter set's factorisation broke down) still leaves the other sets' values."""
        S = int(S)
        nS = (self.n, max(S, 0))
        st, out = self._call_for(self.lib.gpslc_y_loo, {"mean": nS, "var": nS, "lpd": nS, "logpdf": nS[1:]}, want,
                                 S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise)
        return (st, *out.values())

    def y_lgo(self, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, G, labels, want=("mean", "var", "lpd", "logpdf")):
        """gpslc_y_lgo with host arrays as given (None = NULL; ``labels``: n integers in [0, G)): ``(status, lgoMean, lgoVar,
        lgoLpd, logpdf)`` — the outputs named in ``want`` as (n, S) / (n, S) / (G, S) / (S,) arrays, the others None (NULL to
        the library).  The status is returned, not raised, as for ``y_loo``."""
        return self._group_call(self.lib.gpslc_y_lgo, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, G, labels, want)

    def y_kfold(self, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, G, labels, want=("mean", "var", "lpd", "logpdf")):
        """gpslc_y_kfold — ``y_lgo`` for groups of any size: ``(status, cvMean, cvVar, cvLpd, logpdf)``, arguments and outputs as
        there."""
        return self._group_call(self.lib.gpslc_y_kfold, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, G, labels, want)

    def _group_call(self, fn, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, G, labels, want):
        """what y_lgo and y_kfold share: the same signature"""
        S, G = int(S), int(G)
        Sn, Gn = max(S, 0), max(G, 0)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
        if lab is not None and lab.shape != (self.n,):
            raise ValueError(f"labels must have shape ({self.n},), got {lab.shape}")
        st, out = self._call_for(fn, {"mean": (self.n, Sn), "var": (self.n, Sn), "lpd": (Gn, Sn), "logpdf": (Sn,)},
                                 want, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, G,
                                 None if lab is None else lab.ctypes.data_as(_lib.c_int32_p))
        return (st, *out.values())

    GRAD_OUTPUTS = ("dU", "duyLS", "dxyLS", "dtyLS", "dyScale", "dyNoise", "dY", "logpdf")

    def y_logpdf_grad(self, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise, want=GRAD_OUTPUTS):
        """gpslc_y_logpdf_grad with host arrays as given (None = NULL): ``(status, out)`` with ``out`` a dict of the outputs named
        in ``want`` — ``dU`` (n, nU, S), ``duyLS`` (nU, S), ``dxyLS`` (nX, S), ``dtyLS``, ``dyScale``, ``dyNoise``, ``logpdf`` (S,),
        ``dY`` (n, S) — the others None (NULL to the library).  The status is returned, not raised, as for ``y_loo``."""
        S = int(S)
        Sn = max(S, 0)
        shapes = {"dU": (self.n, self.nU, Sn), "duyLS": (self.nU, Sn), "dxyLS": (self.nX, Sn), "dtyLS": (Sn,), "dyScale": (Sn,),
                  "dyNoise": (Sn,), "dY": (self.n, Sn), "logpdf": (Sn,)}          # in GRAD_OUTPUTS' order
        unknown = set(want) - set(shapes)
        if unknown:
            raise ValueError(f"unknown gradient outputs {sorted(unknown)}: choose from {self.GRAD_OUTPUTS}")
        return self._call_for(self.lib.gpslc_y_logpdf_grad, shapes, want, S, U, X_or_none, Y_or_none, uyLS, xyLS, tyLS, yScale, yNoise)

    NODE_GRAD_OUTPUTS = ("dF", "dls", "dscale", "dnoise", "dtarget", "logpdf")

    def nodes_logpdf_grad(self, nodes, want=NODE_GRAD_OUTPUTS):
        """gpslc_nodes_logpdf_grad for a sequence of (F, LS, scale, noise, target) as ``nodesLogpdf`` takes them: ``(status, out)``
        with ``out`` a dict of the outputs named in ``want`` in the library's flat layouts — ``dF`` (n * sum nF,): the nodes'
        (n, nF) column-major blocks one after the other; ``dls`` (sum nF,); ``dscale``, ``dnoise``, ``logpdf`` (count,);
        ``dtarget`` (n, count) — the others None (NULL to the library).  The status is returned, not raised, as for ``y_loo``."""
        unknown = set(want) - set(self.NODE_GRAD_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown gradient outputs {sorted(unknown)}: choose from {self.NODE_GRAD_OUTPUTS}")
        cnt = len(nodes)
        arr, _keep = _marshal_nodes(nodes, self)
        total = sum(int(arr[i].nF) for i in range(cnt))
        shapes = {"dF": (self.n * total,), "dls": (total,), "dscale": (cnt,), "dnoise": (cnt,), "dtarget": (self.n, cnt),
                  "logpdf": (cnt,)}          # in NODE_GRAD_OUTPUTS' order
        return self._call_for(self.lib.gpslc_nodes_logpdf_grad, shapes, want, cnt, C.cast(arr, C.c_void_p))

    def predict_new(self, S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, form, doT, doT_base, pred_noise,
                    want=("mean", "var")):
        """gpslc_predict_new with host arrays as given (None = NULL): ``(status, mean, var, cov)`` — the outputs named in
        ``want`` as (m, S, L) / (m, m, S, L) column-major arrays, the others None (NULL to the library).  ``form`` is "outcome",
        "contrast" or "slope" (or the header's integer).  The status is returned, not raised: a positive one (a sample's
        factorisation broke down) leaves NaN in that sample's outputs and the other samples' values; after a negative one
        the outputs hold nothing."""
        S, m = int(S), int(m)
        L = 0 if doT is None else int(np.size(doT))
        dims = (max(m, 0), max(S, 0), L)
        st, out = self._call_for(self.lib.gpslc_predict_new, {"mean": dims, "var": dims, "cov": (dims[0],) + dims}, want,
                                 S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, int(NEW_FORMS.get(form, form)), L, doT,
                                 doT_base, float(pred_noise), fill=None)      # written in full by every call that returns a status >= 0
        return (st, *out.values())

    def predict_new_vec(self, S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, form, doT, doT_base, pred_noise,
                        want=("mean", "var")):
        """gpslc_predict_new_vec — ``predict_new`` at per-individual levels: ``doT`` (and ``doT_base``) are (m, L) column-major,
        new individual i at level l is set to ``doT[i, l]``.  Forms "outcome" and "contrast"; outputs and status as there."""
        S, m = int(S), int(m)
        L = 0 if doT is None or np.ndim(doT) != 2 else int(np.shape(doT)[1])
        dims = (max(m, 0), max(S, 0), L)
        st, out = self._call_for(self.lib.gpslc_predict_new_vec, {"mean": dims, "var": dims, "cov": (dims[0],) + dims}, want,
                                 S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, int(NEW_FORMS.get(form, form)), L, doT,
                                 doT_base, float(pred_noise), fill=None)      # written in full by every call that returns a status >= 0
        return (st, *out.values())

    def y_test(self, S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xtest, Utest, Ttest, Ytest, want=("mean", "var", "lpd", "joint")):
        """gpslc_y_test with host arrays as given (None = NULL): ``(status, mean, var, lpd, lpd_joint)`` — the outputs named in
        ``want`` as (m, S) / (S,) arrays, the others None (NULL to the library).  The status is returned, not raised, as for
        ``predict_new``."""
        S, m = int(S), int(m)
        mS = (max(m, 0), max(S, 0))
        st, out = self._call_for(self.lib.gpslc_y_test, {"mean": mS, "var": mS, "lpd": mS, "joint": mS[1:]}, want,
                                 S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xtest, Utest, Ttest, Ytest, fill=None)
        return (st, *out.values())

    def predict_new_weighted(self, S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, form, doT, doT_base, weights, pred_noise,
                             want=("mean", "var"), G=None):
        """gpslc_predict_new_weighted with host arrays as given (None = NULL): ``(status, meanW, varW, covW)`` — the outputs named
        in ``want`` as (S, L, G) / (S, L, L, G) column-major arrays, the others None (NULL to the library).  ``weights`` is (G, m)
        (row g = weight column g; a vector: G = 1), ``G`` overrides the count that is passed.  ``form`` and the status are
        ``predict_new``'s: a positive one leaves NaN in that sample's outputs and the other samples' values."""
        S, m = int(S), int(m)
        L = 0 if doT is None else int(np.size(doT))
        W = None if weights is None else np.ascontiguousarray(np.atleast_2d(np.asarray(weights, dtype=np.float64)))   # weights[i + m*g]
        G = int(G) if G is not None else 0 if W is None else W.shape[0]
        dims = (max(S, 0), L, max(G, 0))
        st, out = self._call_for(self.lib.gpslc_predict_new_weighted, {"mean": dims, "var": dims, "cov": dims[:2] + dims[1:]}, want,
                                 S, U, uyLS, xyLS, tyLS, yScale, yNoise, m, Xnew, Unew, int(NEW_FORMS.get(form, form)), L, doT,
                                 doT_base, G, W, float(pred_noise), fill=None)      # written in full by every call that returns a status >= 0
        return (st, *out.values())

    def profile_reset(self):
        self.lib.gpslc_profile_reset(self.h)

    def profile_get(self, kernel_class=0):
        """(launches, ms, algorithmic flop) of the tile-update kernel; class 0 = trailing updates (the dominant
        kernel), 1 = the fused in-panel launches."""
        n = C.c_int64()
        ms = C.c_double()
        fl = C.c_double()
        self.lib.gpslc_profile_get_class(self.h, int(kernel_class), C.byref(n), C.byref(ms), C.byref(fl))
        return n.value, ms.value, fl.value


_scratch_ctx: Optional[Context] = None


def _kernel_ctx() -> Context:
    global _scratch_ctx
    if _scratch_ctx is None:
        _scratch_ctx = Context(1, 0, 0)
    return _scratch_ctx


# ------------------------------------------------------------------------------------------
# src/kernel.jl
# ------------------------------------------------------------------------------------------

def rbfKernelLog(X1, X2, LS):
    """rbfKernelLog(X1, X2, LS) -> n x n (src/kernel.jl:24-32 matrix/vector; :34-42 vector of vectors)."""
    A = np.asarray(X1)
    B = np.asarray(X2)
    if A.dtype == object or B.dtype == object:
        raise TypeError("ragged input")
    if A.shape != B.shape:
        raise AssertionError("X1 and X2 are different sizes!")
    A = _f(A if A.ndim == 2 else A.reshape(A.shape[0], -1))
    B = _f(B if B.ndim == 2 else B.reshape(B.shape[0], -1))
    n, d = A.shape
    ls = np.atleast_1d(np.asarray(LS, dtype=np.float64))
    if ls.shape[0] not in (1, d) or ls.ndim != 1:
        raise AssertionError("vector lengthscale doesn't match individual")
    ls = np.ascontiguousarray(ls)
    out = np.empty((n, n), order="F")
    ctx = _kernel_ctx()
    ctx.check(ctx.lib.gpslc_rbf_log(ctx.h, _p(A), _p(B), n, d, _p(ls), ls.shape[0], _p(out)))
    return out


def rbfKernelLogScalar(Xi, Xiprime, LS):
    """rbfKernelLogScalar(Xi, Xiprime, LS) = -sum((Xi - Xiprime)^2 / LS^2) for one pair of individuals
    (src/kernel.jl:13-19), evaluated by the same device kernel as the matrix form (n = 1)."""
    a = np.atleast_1d(np.asarray(Xi, dtype=np.float64))
    b = np.atleast_1d(np.asarray(Xiprime, dtype=np.float64))
    ls = np.asarray(LS, dtype=np.float64)
    if not (ls.shape == () or ls.shape[0] == a.shape[0]):
        raise AssertionError("vector lengthscale doesn't match individual")
    return float(rbfKernelLog(a[None, :], b[None, :], ls)[0, 0])


def logit(prob):
    """logit(prob) = log(prob / (1 - prob)) (src/kernel.jl:46)."""
    return float(np.log(prob / (1 - prob)))


def expit(x):
    """expit(x) = exp(x) / (1 + exp(x)) (src/kernel.jl:49)."""
    return float(np.exp(x) / (1.0 + np.exp(x)))


def processCov(logCov, scale, noise=None):
    """processCov(logCov, scale[, noise]) (src/kernel.jl:53-59)."""
    lc = _f(np.atleast_2d(logCov))
    n = lc.shape[0]
    if lc.shape != (n, n):
        raise AssertionError("logCov must be square")
    out = np.empty((n, n), order="F")
    ctx = _kernel_ctx()
    ctx.check(ctx.lib.gpslc_process_cov(ctx.h, _p(lc), n, float(scale), 0.0 if noise is None else float(noise),
                                        _p(out)))
    return out


# ------------------------------------------------------------------------------------------
# GPSLCObject: data + the flattened posterior pack extractParameters would produce
# ------------------------------------------------------------------------------------------

@dataclass
class HyperParameters:
    """src/types.jl:22-30 with the defaults of src/hyperparameters.jl:85-102."""
    nU: Optional[int] = 1
    nOuter: int = 24
    nMHInner: int = 10
    nESInner: int = 5
    nBurnIn: int = 10
    stepSize: int = 1
    predictionCovarianceNoise: float = PREDICTION_COVARIANCE_NOISE


@dataclass
class GPSLCObject:
    """Data (X, T, Y) plus the posterior samples in flat form.

    ``U`` (n, nU, S), ``uyLS`` (nU, S), ``xyLS`` (nX, S), ``tyLS``/``yNoise``/``yScale`` (S,) are the
    values ``extractParameters(g, i)`` (src/utils.jl:92-124) returns for i in nBurnIn:stepSize:nOuter
    (burn-in index inclusive, src/estimation.jl:72,78), stacked along the last axis.  ``U``/``uyLS``
    are None for the models without latent confounders, ``X``/``xyLS`` None without covariates.
    """
    X: Optional[np.ndarray]
    T: np.ndarray
    Y: np.ndarray
    U: Optional[np.ndarray]
    uyLS: Optional[np.ndarray]
    xyLS: Optional[np.ndarray]
    tyLS: np.ndarray
    yNoise: np.ndarray
    yScale: np.ndarray
    hyperparams: HyperParameters = field(default_factory=HyperParameters)
    device: int = 0
    fp32_kernel: bool = False   # GPSLC_FLAG_FP32_KERNEL: RBF evaluation in fp32, factorisation in fp64
    _ctx: Optional[Context] = field(default=None, repr=False)

    def __post_init__(self):
        self.T = _f(self.T).reshape(-1)
        self.Y = _f(self.Y).reshape(-1)
        n = self.Y.shape[0]
        if self.T.shape[0] != n:
            raise AssertionError("size(T, 1) != n")
        if self.X is not None:
            self.X = _f(self.X).reshape(n, -1, order="F")
        self.tyLS = np.ascontiguousarray(np.atleast_1d(self.tyLS), dtype=np.float64)
        S = self.tyLS.shape[0]
        self.yNoise = np.ascontiguousarray(np.atleast_1d(self.yNoise), dtype=np.float64)
        self.yScale = np.ascontiguousarray(np.atleast_1d(self.yScale), dtype=np.float64)
        if self.U is not None:
            U = np.asarray(self.U, dtype=np.float64)
            if U.ndim == 2:
                U = U[:, :, None] if S == 1 else U[:, None, :]
            self.U = np.asfortranarray(U)
            if self.U.shape[0] != n or self.U.shape[2] != S:
                raise AssertionError("size(U, 1) != n")
            self.uyLS = np.asfortranarray(np.asarray(self.uyLS, dtype=np.float64).reshape(self.U.shape[1], S, order="F"))
        if self.X is not None:
            self.xyLS = np.asfortranarray(np.asarray(self.xyLS, dtype=np.float64).reshape(self.X.shape[1], S, order="F"))

    # ---- size getters, src/utils.jl:130-161
    def getN(self):
        return self.Y.shape[0]

    def getNX(self):
        return 0 if self.X is None else self.X.shape[1]

    def getNU(self):
        return 0 if self.U is None else self.U.shape[1]

    def getNumPosteriorSamples(self):
        return self.tyLS.shape[0]

    def ctx(self) -> Context:
        if self._ctx is None:
            c = Context(self.getN(), self.getNX(), self.getNU(), device=self.device, fp32_kernel=self.fp32_kernel)
            c.set_data(self.X, self.T, self.Y)
            self._ctx = c
        return self._ctx

    def _params(self):
        return (_p(self.U), _p(self.uyLS), _p(self.xyLS), _p(self.tyLS), _p(self.yScale), _p(self.yNoise))

    def ctxs(self, devices: Sequence[int]):
        """One context per entry of ``devices`` (repeats allowed: distinct contexts on one GPU), each holding the data —
        what ``gpslc_predict_multi`` shards the posterior samples over.  Cached per device list."""
        key = tuple(int(d) for d in devices)
        if not key:
            raise AssertionError("devices must name at least one GPU")
        cache = self.__dict__.setdefault("_multi", {})
        if key not in cache:
            cs = []
            for d in key:
                c = Context(self.getN(), self.getNX(), self.getNU(), device=d, fp32_kernel=self.fp32_kernel)
                c.set_data(self.X, self.T, self.Y)
                cs.append(c)
            cache[key] = cs
        return cache[key]


def getN(g):
    return g.getN()


def getNX(g):
    return g.getNX()


def getNU(g):
    return g.getNU()


def getNumPosteriorSamples(g):
    return g.getNumPosteriorSamples()


def _single(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y) -> GPSLCObject:
    if U is not None:
        U = np.asarray(U, dtype=np.float64)
        U = U.reshape(U.shape[0], -1)[:, :, None]
        uyLS = np.atleast_1d(np.asarray(uyLS, dtype=np.float64))[:, None]
    if X is not None:
        X = np.asarray(X, dtype=np.float64)
        X = X.reshape(X.shape[0], -1)
        xyLS = np.atleast_1d(np.asarray(xyLS, dtype=np.float64))[:, None]
    return GPSLCObject(X, T, Y, U, uyLS, xyLS, [tyLS], [yNoise], [yScale])


# ------------------------------------------------------------------------------------------
# src/estimation.jl
# ------------------------------------------------------------------------------------------

def likelihoodDistribution(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, doT):
    """likelihoodDistribution(...) -> (Y, CovWW, CovWWs, CovWWp, CovC11, CovC12, CovC21, CovC22)
    (src/likelihood.jl:8-174; the method is chosen by which of U / X is None, like the reference's dispatch)."""
    g = _single(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y)
    n = g.getN()
    x, d = _intervention(doT, n)
    ctx = g.ctx()
    outs = [np.empty((n, n), order="F") for _ in range(7)]
    if d is None:
        st = ctx.lib.gpslc_likelihood_distribution(ctx.h, _p(g.U), _p(g.uyLS), _p(g.xyLS), float(tyLS), float(yScale),
                                                   float(yNoise), x, *[_p(o) for o in outs])
    else:
        st = ctx.lib.gpslc_likelihood_distribution_vec(ctx.h, _p(g.U), _p(g.uyLS), _p(g.xyLS), float(tyLS), float(yScale),
                                                       float(yNoise), _p(d), *[_p(o) for o in outs])
    ctx.check(st)
    return (g.Y.copy(), *outs)


def extractParameters(g: "GPSLCObject", posteriorSampleIdx: int):
    """extractParameters(g, i) -> (uyLS, xyLS, tyLS, yNoise, yScale, U) (src/utils.jl:92-124); ``i`` is
    1-based like the reference, counting the retained posterior samples."""
    i = int(posteriorSampleIdx) - 1
    if not 0 <= i < g.getNumPosteriorSamples():
        raise IndexError("posterior sample index out of range")   # Julia: BoundsError
    return (None if g.uyLS is None else g.uyLS[:, i].copy(), None if g.xyLS is None else g.xyLS[:, i].copy(),
            float(g.tyLS[i]), float(g.yNoise[i]), float(g.yScale[i]), None if g.U is None else g.U[:, :, i].copy())


def conditionalITE(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, doT):
    """conditionalITE(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y, doT) -> MeanITE (n,), CovITE (n, n)
    (src/estimation.jl:36-50; no jitter, like the reference)."""
    g = _single(uyLS, xyLS, tyLS, yNoise, yScale, U, X, T, Y)
    M, Cv = _ite_distributions(g, doT, 0.0)
    return M[0], Cv[0]


def _ite_distributions(g: GPSLCObject, doT, pred_noise, want_cov=True, baseline=None, slope=False, outcome=False):
    p = _plan(g, _levels(g, doT), "distributions", baseline=baseline, slope=slope, outcome=outcome)
    n, S = g.getN(), g.getNumPosteriorSamples()
    sym, opt = _symbol(p)
    ctx = g.ctx()
    M = np.empty((S, n), order="F")
    Cv = np.empty((S, n, n), order="F") if want_cov else None
    level = _p(p.levels[:, 0]) if p.vec else float(p.levels[0])           # one level: the n values, or the scalar by value
    base = (float(p.base[0]),) if "base" in opt else ()
    ctx.check(getattr(ctx.lib, sym)(ctx.h, S, *g._params(), level, *base, float(pred_noise), _p(M), _p(Cv)))
    return M, Cv


def ITEDistributions(g: GPSLCObject, doT, baseline=None, slope=False, outcome=False):
    """MeanITEs (S, n), CovITEs (S, n, n) incl. + I*predictionCovarianceNoise (src/estimation.jl:66-86).  ``baseline`` = a
    scalar b: the contrast f(doT) - f(b) of two scalar levels instead of f(doT) - f(T) (gpslc_ite_distributions_contrast).
    ``slope=True``: the marginal effect d f_i(t) / dt at the scalar t = doT (gpslc_ite_distributions_slope; see predict).
    ``outcome=True``: the potential outcome f_i(doT) itself, doT a scalar or a per-individual vector — mean D alpha and covariance
    CovC22 of src/likelihood.jl:49, + I*predictionCovarianceNoise (gpslc_ite_distributions_outcome[_vec]; see predict)."""
    return _ite_distributions(g, doT, g.hyperparams.predictionCovarianceNoise, baseline=baseline, slope=slope, outcome=outcome)


def conditionalSATE(MeanITE, CovITE):
    """src/estimation.jl:116-121 (pure reduction; kept on the host for API parity)."""
    n = MeanITE.shape[0]
    return float(np.sum(MeanITE) / n), float(np.sum(CovITE) / n ** 2)


def SATEDistributions(g: GPSLCObject, doT, baseline=None, weights=None, slope=False, outcome=False):
    """MeanSATEs (S,), VarSATEs (S,) (src/estimation.jl:127-140) — O(N^2) per sample on the GPU,
    without materialising CovITE.  ``baseline`` = a scalar b: the contrast doT against b (see predict).  ``weights`` = a
    length-n vector: the weighted effect w' ITE instead of the average over everybody, same shapes; a (G, n) array: (S, G)
    each (see predict).  ``slope=True``: the average marginal effect at the scalar doT (see predict).
    ``outcome=True``: the average potential outcome — the dose-response function at the scalar doT, the value of the policy for
    a per-individual doT (see predict)."""
    m, v, _ = predict(g, _levels(g, doT), baseline=baseline, weights=weights, slope=slope, outcome=outcome)
    return m[:, 0].copy(), v[:, 0].copy()


def SATEsamples(MeanSATEs, VarSATEs, nSamplesPerMixture, z=None, seed=0):
    """src/estimation.jl:148-163 (variance passed as sigma, :159)."""
    lib = _lib.load()
    m = np.ascontiguousarray(MeanSATEs, dtype=np.float64)
    v = np.ascontiguousarray(VarSATEs, dtype=np.float64)
    S = m.shape[0]
    out = np.empty(S * nSamplesPerMixture)
    zz = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
    st = lib.gpslc_sate_samples(_p(m), _p(v), S, int(nSamplesPerMixture), int(seed), _p(zz), _p(out))
    if st != 0:
        raise GPSLCError(st, "gpslc_sate_samples")
    return out


def _levels(g: GPSLCObject, doT):
    """One intervention as the ``doTs`` of predict: [x] for a scalar, a (1, n) array for a per-individual vector."""
    x, d = _intervention(doT, g.getN())
    return [x] if d is None else d[None, :]


def predict(g: GPSLCObject, doTs, want_mean_ite=False, spp=0, z=None, seed=0,
            want_draws=False, devices: Optional[Sequence[int]] = None, baseline=None, weights=None, slope=False,
            outcome=False):
    """The ensemble entry point (gpslc_predict): returns MeanSATE (S, L), VarSATE (S, L) and, when
    asked, MeanITE (n, S, L) / draws (L, n, S*spp).  ``doTs``: L scalar levels (1-D), or an (L, n) array of L per-individual
    intervention vectors (gpslc_predict_vec).  ``devices`` = a list of GPU indices shards the posterior samples
    over one context per entry through ``gpslc_predict_multi`` (same results, bit for bit; scalar levels only).
    ``baseline`` = a scalar or L values b: level l becomes the contrast f(doTs[l]) - f(b[l]) between two scalar levels
    (gpslc_predict_contrast: "treatment a against treatment b", with its own covariance and draws) instead of
    f(doTs[l]) - f(T); ``None`` is the plain call.  Scalar levels and one GPU only.
    ``weights`` = a length-n vector or a (G, n) array: the first two results become the weighted effects tau_w = w' ITE —
    mean w' MeanITE and variance w' (CovITE + predictionCovarianceNoise I) w, the weights used as given (gpslc_predict_weighted;
    no n x n covariance is formed) — of shape (S, L) for a vector and (S, L, G) for an array.  Float rows are taken as they are
    (1/n everywhere is the SATE, a difference of two group averages the difference of two groups with its correct variance);
    a Bool row is a group mask and means that group's average (``groupWeights`` builds them from labels).  With ``baseline``
    the weighted contrast: a binary treatment, ``predict(g, [1.0], baseline=0.0, weights=(T == 1))`` is the ATT.  MeanITE and
    the draws are unchanged.  Scalar levels and one GPU only.
    ``slope=True``: level l becomes the marginal effect d f_i(t) / dt at t = doTs[l], everybody set to that dose
    (gpslc_predict_slope) — MeanSATE / VarSATE its average over the population, the slope of the dose-response curve, MeanITE and
    the draws the per-individual slope; exact (the derivative of the Gaussian process, nothing is differenced).  Combines with
    ``weights``; ``baseline``, vector levels and ``devices`` raise ValueError.
    ``outcome=True``: level l becomes the potential outcome mu_i = f_i(doTs[l]) itself, the response surface and not a difference
    of it (gpslc_predict_outcome) — MeanSATE / VarSATE its average over the population, the average dose-response function mu(a)
    (E[Y(1)], E[Y(0)] for a binary treatment), MeanITE and the draws the per-individual outcome.  With an (L, n) array of
    per-individual levels (gpslc_predict_outcome_vec) MeanSATE / VarSATE are the value of the treatment policy doTs[l] and its
    variance; doTs[l] = T gives the fitted surface.  The prior mean is zero as in the reference's model: far from the data the
    outcome returns to 0, not to the sample mean of Y.  This is the latent surface; the predictive distribution of a new
    observation adds yNoise to the diagonal, which is left to the caller.  Combines with ``weights`` for scalar levels;
    ``baseline`` (the contrast IS the difference of two outcomes), ``slope``, ``devices`` and ``weights`` with vector levels
    raise ValueError."""
    p = _plan(g, doTs, "predict", baseline=baseline, weights=weights, slope=slope, outcome=outcome, devices=devices)
    ms, vs, _, mi, dr = _run(g, p, want_mean_ite, spp, z, seed, want_draws, False)
    if p.wvec:
        ms, vs = ms[:, :, 0], vs[:, :, 0]
    if want_draws:
        return ms, vs, mi, dr
    return ms, vs, mi


def _run(g: GPSLCObject, p: _Plan, want_mean_ite, spp, z, seed, want_draws, want_cov):
    """Allocate the outputs of a ``predict`` / ``curve`` plan, check ``z``, call the plan's symbol: (mean, var, covW or None,
    MeanITE or None, draws or None), the first two (S, L) without weights and (S, L, G) with."""
    n, S, L = g.getN(), g.getNumPosteriorSamples(), p.L
    sym, opt = _symbol(p)
    cs = [g.ctx()] if p.devices is None else g.ctxs(p.devices)
    ctx = cs[0]
    G = p.W.shape[0] if p.weighted else 0
    ms, vs = (np.empty((S, L, G) if p.weighted else (S, L), order="F") for _ in range(2))
    cw = np.empty((S, L, L, G), order="F") if want_cov else None
    mi = np.empty((n, S, L), order="F") if want_mean_ite else None
    dr = np.empty((L, n, S * spp), order="F") if want_draws else None
    zz = None
    if z is not None:
        zz = _f(z)
        if zz.shape != (n, spp, S, L):
            raise AssertionError(f"z must be (n, spp, S, L) = {(n, spp, S, L)}, got {zz.shape}")
    st = getattr(ctx.lib, sym)(
        *((len(cs), (C.c_void_p * len(cs))(*[c.h for c in cs])) if "multi" in opt else (ctx.h,)),
        S, *g._params(), L, _p(p.levels),
        *((_p(p.base),) if "base" in opt else ()),
        *((G, _p(p.W)) if "weights" in opt else ()),
        float(g.hyperparams.predictionCovarianceNoise), int(spp), int(seed), _p(zz), _p(ms), _p(vs),
        *((_p(cw),) if "cov" in opt else ()),
        _p(mi), _p(dr),
        *((None,) if "multi" in opt else ()))
    ctx.check(st)
    return ms, vs, cw, mi, dr


def _predict_curve(g: GPSLCObject, doTs, baseline=None, weights=None, want_mean_ite=False, spp=0, z=None, seed=0,
                   want_draws=False, want_cov=True, devices=None, slope=False, outcome=False):
    """gpslc_predict_curve: (meanW (S, L, G), varW (S, L, G), covW (S, L, L, G) or None, MeanITE or None, draws or None) and
    whether ``weights`` was a single vector.  ``weights=None`` is 1/n for everybody.  ``slope=True``: gpslc_predict_slope's
    weighted form; ``outcome=True``: gpslc_predict_outcome's."""
    p = _plan(g, doTs, "curve", baseline=baseline, weights=weights, slope=slope, outcome=outcome, devices=devices)
    return _run(g, p, want_mean_ite, spp, z, seed, want_draws, want_cov), p.wvec


def effectCurve(g: GPSLCObject, doTs, baseline=None, weights=None, devices=None, slope=False, outcome=False):
    """The weighted effect over a sweep of L scalar levels as ONE Gaussian: mean (S, L[, G]) and the joint covariance
    cov (S, L, L[, G]) of tau_l = w' ITE_l across the levels, per posterior sample (gpslc_predict_curve).  The diagonal of
    ``cov`` is the ``var`` of ``predict`` to the bits; the off-diagonal blocks are what simultaneous bands, comparisons of
    two levels and functionals of the curve (slope, maximum, area) need.  ``weights=None`` means 1/n, the SATE curve; a
    length-n vector or a (G, n) array as in ``predict`` (a (G, n) array adds the trailing group axis); ``baseline`` as in
    ``predict``.  ``slope=True``: the curve of average marginal effects, tau_l = w' (d f / dt at doTs[l]) — the derivative of the
    dose-response curve with its joint covariance (``weights=None`` is 1/n here too).  ``outcome=True``: the average dose-response curve itself,
    tau_l = w' f(doTs[l]), with its joint covariance across the levels — the curve of levels, where the default is the curve of
    effects.  Scalar levels and one GPU only."""
    (mw, _, cw, _, _), wvec = _predict_curve(g, doTs, baseline=baseline, weights=weights, devices=devices, slope=slope,
                                             outcome=outcome)
    if wvec:
        return mw[:, :, 0], cw[:, :, :, 0]
    return mw, cw


def curveSamples(mean, cov, samplesPerPosterior, z=None, seed=0):
    """Joint draws of curves from ``effectCurve``'s (mean (S, L, G), cov (S, L, L, G)): (L, spp, S, G), draw d of sample s and
    group g at [:, d, s, g] (gpslc_curve_samples: pivoted Cholesky per block, semi-definite blocks allowed).  ``z``: (L, spp,
    S, G) standard normals, else the library's Philox stream ``seed``."""
    lib = _lib.load()
    m, c = _f(mean), _f(cov)
    if m.ndim != 3 or c.shape != (m.shape[0], m.shape[1], m.shape[1], m.shape[2]):
        raise ValueError(f"mean must be (S, L, G) and cov (S, L, L, G), got {m.shape} and {c.shape}")
    S, L, G = m.shape
    spp = int(samplesPerPosterior)
    zz = None
    if z is not None:
        zz = _f(z)
        if zz.shape != (L, spp, S, G):
            raise ValueError(f"z must be (L, spp, S, G) = {(L, spp, S, G)}, got {zz.shape}")
    out = np.empty((L, spp, S, G), order="F")
    st = lib.gpslc_curve_samples(_p(m), _p(c), S, L, G, spp, int(seed), _p(zz), _p(out))
    if st != 0:
        raise GPSLCError(st, "gpslc_curve_samples")
    return out


def sampleEffectCurve(g: GPSLCObject, doTs, samplesPerPosterior=10, z=None, seed=0, baseline=None, weights=None, devices=None,
                      slope=False, outcome=False):
    """Joint draws of the effect curve over the L levels: (L, S*spp), column order sample-outer / draw-inner as sampleSATE, or
    (G, L, S*spp) for a (G, n) weight array.  Unlike sampleSATE per level, the L values of a column are ONE draw of the curve
    (they share the Gaussian process).  ``z``: (L, spp, S[, G]) standard normals, else the Philox stream ``seed``.
    ``slope=True``: draws of the curve of average marginal effects; ``outcome=True``: draws of the dose-response curve (see
    effectCurve)."""
    (mw, _, cw, _, _), wvec = _predict_curve(g, doTs, baseline=baseline, weights=weights, devices=devices, slope=slope,
                                             outcome=outcome)
    S, L, G = mw.shape
    spp = int(samplesPerPosterior)
    if z is not None:
        z = np.asarray(z, dtype=np.float64)
        if wvec and z.ndim == 3:
            z = z[:, :, :, None]
    dr = curveSamples(mw, cw, spp, z=z, seed=seed)                      # (L, spp, S, G)
    out = np.transpose(dr.reshape(L, spp * S, G, order="F"), (2, 0, 1))     # column d + spp*s
    return np.ascontiguousarray(out[0]) if wvec else np.ascontiguousarray(out)


def ITEsamples(g_or_means, doT_or_covs, nSamplesPerMixture, z=None, seed=0, baseline=None, slope=False, outcome=False):
    """ITEsamples: n x (S*spp) draws, column order sample-outer / draw-inner (src/estimation.jl:95-109).
    Called as ITEsamples(g, doT, spp): the factor of CovITE + jitter is computed once per sample on the GPU.
    ``baseline`` = a scalar b: draws of the contrast doT against b (see predict).  ``slope=True``: draws of the per-individual
    marginal effect at the scalar doT (see predict).  ``outcome=True``: draws of the per-individual potential outcome at the
    scalar or per-individual doT (see predict)."""
    g, doT = g_or_means, doT_or_covs
    zz = None
    if z is not None:   # z given in the reference's (n, S*spp) column order
        n, S = g.getN(), g.getNumPosteriorSamples()
        # column j*spp + d  ->  [i, d, j] under a column-major reshape
        zz = np.asarray(z, dtype=np.float64).reshape(n, nSamplesPerMixture, S, order="F")[:, :, :, None]
    _, _, _, dr = predict(g, _levels(g, doT), spp=nSamplesPerMixture, z=zz, seed=seed, want_draws=True, baseline=baseline,
                          slope=slope, outcome=outcome)
    return np.asfortranarray(dr[0])


# ------------------------------------------------------------------------------------------
# src/driver.jl, src/prediction.jl
# ------------------------------------------------------------------------------------------

def sampleITE(g: GPSLCObject, doT, samplesPerPosterior=10, z=None, seed=0, baseline=None, slope=False, outcome=False):
    """sampleITE(g, doT; samplesPerPosterior=10) -> n x (S*spp) (src/driver.jl:86-89); ``baseline``: the contrast doT
    against that scalar level; ``slope=True``: the marginal effect at the scalar doT; ``outcome=True``: the potential outcome
    at doT itself."""
    return ITEsamples(g, doT, samplesPerPosterior, z=z, seed=seed, baseline=baseline, slope=slope, outcome=outcome)


def sampleSATE(g: GPSLCObject, doT, samplesPerPosterior=10, z=None, seed=0, baseline=None, weights=None, slope=False,
               outcome=False):
    """sampleSATE(g, doT; samplesPerPosterior=10) -> (S*spp,) (src/driver.jl:108-111); ``baseline``: the contrast doT
    against that scalar level.  ``weights`` = a length-n vector: samples of the weighted effect, (S*spp,); a (G, n) array:
    (G, S*spp), row g from SATEsamples of group g's means and variances with ``z[g]`` (``z``: (G, S*spp), or (S*spp,) shared
    by every group) or the Philox seed ``seed + g``.  ``slope=True``: samples of the average marginal effect at the scalar doT.
    ``outcome=True``: samples of the average potential outcome (the policy value for a per-individual doT)."""
    m, v = SATEDistributions(g, doT, baseline=baseline, weights=weights, slope=slope, outcome=outcome)
    if m.ndim == 1:
        return SATEsamples(m, v, samplesPerPosterior, z=z, seed=seed)
    zz = None if z is None else np.broadcast_to(np.asarray(z, dtype=np.float64), (m.shape[1], m.shape[0] * samplesPerPosterior))
    return np.stack([SATEsamples(m[:, k], v[:, k], samplesPerPosterior, z=None if zz is None else zz[k], seed=seed + k)
                     for k in range(m.shape[1])])


def doTRange(minDoT, maxDoT, fidelity):
    """``minDoT:(|maxDoT-minDoT|/fidelity):maxDoT`` (src/prediction.jl:24-28)."""
    delta = abs(maxDoT - minDoT)
    step = delta / fidelity
    if step == 0:
        raise ValueError("range step cannot be zero")
    if maxDoT < minDoT:
        return np.zeros(0)
    npts = int(np.floor((maxDoT - minDoT) / step + 1e-9)) + 1
    return minDoT + step * np.arange(npts)


def predictCounterfactualEffects(g: GPSLCObject, nSamplesPerMixture, fidelity=100, minDoT=None, maxDoT=None,
                                 z=None, seed=0, devices: Optional[Sequence[int]] = None, outcome=False):
    """predictCounterfactualEffects(g, spp; fidelity, minDoT, maxDoT) -> (ite [L, n, S*spp], doTrange)
    (src/prediction.jl:23-36).  All levels share one factorisation of A per posterior sample; ``devices`` shards the
    posterior samples over several GPUs (``gpslc_predict_multi``).  ``outcome=True``: draws of every individual's outcome
    surface f_i(a) over the sweep instead of the effects f_i(a) - f_i(T_i) (one GPU only)."""
    _refuse("predict", outcome=outcome, devices=devices)
    lo = float(np.min(g.T)) if minDoT is None else float(minDoT)
    hi = float(np.max(g.T)) if maxDoT is None else float(maxDoT)
    rng = doTRange(lo, hi, fidelity)
    zz = None
    if z is not None:   # (L, n, S*spp) in the reference's order
        n, S = g.getN(), g.getNumPosteriorSamples()
        L = rng.shape[0]
        zz = np.asarray(z, dtype=np.float64).reshape(L, n, nSamplesPerMixture, S, order="F")
        zz = np.transpose(zz, (1, 2, 3, 0))
    _, _, _, dr = predict(g, rng, spp=nSamplesPerMixture, z=zz, seed=seed, want_draws=True, devices=devices, outcome=outcome)
    return dr, rng


def mvnDraw(cov, z, covscale=None, ctx: Optional[Context] = None):
    """chol(covscale_s * cov) z_s per column of ``z`` (gpslc_mvn_draw): Gen's `mvnormal(zeros(n), uCov)` — the auxiliary vector
    of `elliptical_slice(trace, :U => k => :U, zeros(n), uCov)` (src/inference.jl:48-54) and the prior draw of
    generateUfromSigmaU (src/model_likelihood.jl:4-10) — with the host's normals.  ``cov=None`` re-uses the covariance cached in
    ``ctx`` (mvnLogpdf caches SigmaU once per data set)."""
    z = _f(z)
    if z.ndim == 1:
        z = z[:, None]
    n, S = z.shape
    covf = None
    if cov is not None:
        cov = np.asarray(cov, dtype=np.float64)
        covf = cov if cov.flags.f_contiguous or cov.flags.c_contiguous else np.ascontiguousarray(cov)  # symmetric
    cs = None if covscale is None else np.ascontiguousarray(np.atleast_1d(covscale), dtype=np.float64)
    ctx = ctx or Context(n, 0, 0)
    out = np.empty((n, S), order="F")
    ctx.check(ctx.lib.gpslc_mvn_draw(ctx.h, S, _p(covf), _p(cs), _p(z), _p(out)))
    return out


def summarizeEstimates(samples, credible_interval=0.90):
    """summarizeEstimates(samples; credible_interval=0.90) (src/driver.jl:129-149): Individual, Mean,
    LowerBound, UpperBound per row of the n x m sample matrix, computed on the GPU (Julia's type-7 quantile: in-LDS
    sort per individual up to 16384 samples per row, exact radix select beyond)."""
    s = _f(np.atleast_2d(samples))
    n, m = s.shape
    mean, lo, hi = np.empty(n), np.empty(n), np.empty(n)
    ctx = _kernel_ctx()
    ctx.check(ctx.lib.gpslc_summarize(ctx.h, _p(s), n, m, float(credible_interval), _p(mean), _p(lo), _p(hi)))
    return {"Individual": np.arange(1, n + 1), "Mean": mean, "LowerBound": lo, "UpperBound": hi}


# ------------------------------------------------------------------------------------------
# src/model_likelihood.jl :Y node
# ------------------------------------------------------------------------------------------

def _overrides(g: GPSLCObject, X_override, Y_override):
    """the overrides of the outcome-model calls as the library takes them (None: the context's data)"""
    return (None if X_override is None else _f(X_override).reshape(g.getN(), g.getNX(), order="F"),
            None if Y_override is None else _f(Y_override, (g.getN(),)))


def yLogpdf(g: GPSLCObject, X_override=None, Y_override=None):
    """log N(y; 0, Ycov) for every parameter set of ``g`` (the score the :Y address contributes to a
    Gen trace; src/model_likelihood.jl:83-120).  ``y`` is ``Y_override`` when given (the value Gen hands to a
    distribution's logpdf), else the data Y the node is constrained to."""
    S = g.getNumPosteriorSamples()
    ctx = g.ctx()
    out = np.empty(S)
    Xo, Yo = _overrides(g, X_override, Y_override)
    U, uy, xy, ty, ys, yn = g._params()
    st = ctx.lib.gpslc_y_logpdf(ctx.h, S, U, _p(Xo), _p(Yo), uy, xy, ty, ys, yn, _p(out))
    ctx.check(st)
    return out


def looPredictive(g: GPSLCObject, X_override=None, Y_override=None):
    """Leave-one-out predictive distribution of every observation under the outcome model of every posterior sample
    (gpslc_y_loo; Rasmussen & Williams §5.4.2) -> ``(mean, var, lpd)``, each (n, S): mean and variance of Y_i given all the
    other observations (``var`` is for the observation: it includes yNoise) and the log density of Y_i under that predictive.
    Each sample conditions on its own hyper-parameters and U, which were inferred with Y_i present.  Overrides and errors as
    ``yLogpdf``: ``Y_override`` is the outcome vector being checked, a failed factorisation raises ``PosDefException``."""
    ctx = g.ctx()
    st, mean, var, lpd, _ = ctx.y_loo(g.getNumPosteriorSamples(), g.U, *_overrides(g, X_override, Y_override), g.uyLS, g.xyLS,
                                      g.tyLS, g.yScale, g.yNoise, want=("mean", "var", "lpd"))
    ctx.check(st)
    return mean, var, lpd


def yLogpdfGrad(g: GPSLCObject, X_override=None, Y_override=None, log_params=False):
    """Gradient of ``yLogpdf`` for every posterior sample (gpslc_y_logpdf_grad; Rasmussen & Williams §5.4.1) -> a dict: ``dU``
    (n, nU, S), ``duyLS`` (nU, S), ``dxyLS`` (nX, S), ``dtyLS``, ``dyScale``, ``dyNoise`` (S,), ``dY`` (n, S) — each in the layout
    of what it differentiates — and ``logpdf`` (S,), the score from the same factorisation.  What a gradient-based move on U and
    the hyper-parameters (HMC, MALA, MAP), a type-II maximum-likelihood start or a sensitivity check of a posterior sample
    needs.  ``log_params=True``: the five positive parameters' gradients are with respect to their logarithms (multiplied by
    the parameter, on the host); ``dU`` and ``dY`` are unchanged.  Overrides and errors as ``yLogpdf``; an fp32 context is
    refused."""
    ctx = g.ctx()
    st, out = ctx.y_logpdf_grad(g.getNumPosteriorSamples(), g.U, *_overrides(g, X_override, Y_override), g.uyLS, g.xyLS, g.tyLS,
                                g.yScale, g.yNoise)
    ctx.check(st)
    if log_params:
        for k, par in (("duyLS", g.uyLS), ("dxyLS", g.xyLS), ("dtyLS", g.tyLS), ("dyScale", g.yScale), ("dyNoise", g.yNoise)):
            if par is not None and out[k].size:       # a model without U (without X) has no uyLS (xyLS): its block stays empty
                out[k] = out[k] * _f(par).reshape(out[k].shape, order="F")
    return out


def _predictive_summary(g: GPSLCObject, Y_override, mean, var, lpd, rows=None):
    """what looSummary, lgoSummary and testSummary share -> (elpd (S,), log mean_s exp(lpd) per row of lpd, zscore (n, S), pit
    (n,)); ``rows``: the outcomes are those of that many other individuals (a test set), not of the n in the data"""
    from math import erf
    Y = g.Y if Y_override is None else _f(Y_override, (g.getN() if rows is None else rows,))
    z = (Y[:, None] - mean) / np.sqrt(var)
    top = np.max(lpd, axis=1)
    rowwise = top + np.log(np.mean(np.exp(lpd - top[:, None]), axis=1))
    pit = np.mean(0.5 * (1.0 + np.vectorize(erf)(z / np.sqrt(2.0))), axis=1)
    return np.sum(lpd, axis=0), rowwise, z, pit


def looSummary(g: GPSLCObject, X_override=None, Y_override=None, loo=None):
    """Summaries of ``looPredictive`` (host arithmetic only; ``loo`` = its result, to summarise one already computed):

    ``elpd`` (S,): sum_i lpd[i, s], the LOO log predictive density of every posterior sample — compare models (nU = 0 / 1 / 2,
    with / without X) on it; ``pointwise`` (n,): log mean_s exp(lpd[i, s]), the individuals the surface misses;
    ``zscore`` (n, S): (Y - mean) / sqrt(var); ``pit`` (n,): mean_s Phi(zscore), uniform on (0, 1) for a calibrated model."""
    elpd, pointwise, z, pit = _predictive_summary(g, Y_override, *(looPredictive(g, X_override, Y_override) if loo is None else loo))
    return {"elpd": elpd, "pointwise": pointwise, "zscore": z, "pit": pit}


def _group_labels(g: GPSLCObject, groups, who="lgoPredictive"):
    """``groups`` (None: the object's ``obj`` column) -> (keys, labels): the distinct group keys in ``np.unique``'s order and
    the int32 label in [0, len(keys)) of every individual"""
    n = g.getN()
    if groups is None:
        groups = getattr(g, "obj", None)
        if groups is None:
            raise ValueError(who + ": this object has no `obj` column to take the groups from; pass groups= (one label per "
                             "individual, e.g. foldLabels(n, K, seed) for K-fold cross-validation)")
    groups = np.asarray(groups)
    if groups.shape != (n,):
        raise ValueError(f"groups must have one label per individual: shape ({n},), got {groups.shape}")
    keys, labels = np.unique(groups, return_inverse=True)
    return keys, np.ascontiguousarray(labels.reshape(n), dtype=np.int32)


def lgoPredictive(g: GPSLCObject, groups=None, X_override=None, Y_override=None):
    """Leave-group-out predictive distribution under the outcome model of every posterior sample (gpslc_y_lgo; Rasmussen &
    Williams §5.4.2 in block form) -> ``(mean, var, lpd, keys)``: a whole group — by default an object of the hierarchical
    data (``g.obj``), with ``groups=foldLabels(n, K, seed)`` a cross-validation fold, or any length-n labelling (ints, strings)
    — is removed and its members predicted jointly from everybody else.  ``mean``, ``var`` (n, S): mean and marginal variance
    (for the observation: yNoise included) of Y_i given all individuals outside i's group; ``lpd`` (G, S): the joint log
    density of each group's outcomes under that predictive, row j belonging to group ``keys[j]`` (the distinct labels,
    sorted).  A group has at most 128 members: ``kfoldPredictive`` takes groups of any size (5 or 10 folds at any n).  Overrides
    and errors as ``looPredictive``."""
    keys, labels = _group_labels(g, groups)
    ctx = g.ctx()
    st, mean, var, lpd, _ = ctx.y_lgo(g.getNumPosteriorSamples(), g.U, *_overrides(g, X_override, Y_override), g.uyLS, g.xyLS,
                                      g.tyLS, g.yScale, g.yNoise, len(keys), labels, want=("mean", "var", "lpd"))
    ctx.check(st)
    return mean, var, lpd, keys


def foldLabels(n, K, seed=0):
    """Labels of K random cross-validation folds of near-equal size (sizes differ by at most one) for n individuals -> (n,)
    int32 in [0, K): a random permutation dealt round-robin.  Pass as ``lgoPredictive(g, groups=...)`` (folds of at most 128
    members) or take ``kfoldPredictive(g, K=K, seed=seed)``."""
    n, K = int(n), int(K)
    if not 1 <= K <= n:
        raise ValueError(f"foldLabels needs 1 <= K <= n, got K = {K}, n = {n}")
    labels = np.empty(n, dtype=np.int32)
    labels[np.random.default_rng(seed).permutation(n)] = np.arange(n, dtype=np.int32) % K
    return labels


def lgoSummary(g: GPSLCObject, groups=None, X_override=None, Y_override=None, lgo=None):
    """Summaries of ``lgoPredictive`` (host arithmetic only; ``lgo`` = its result, to summarise one already computed):

    ``elpd`` (S,): sum_g lpd[g, s], the leave-group-out log predictive density of every posterior sample — the score to compare
    models (nU = 0 / 1 / 2) on for hierarchical data; ``groupwise`` (G,): log mean_s exp(lpd[g, s]), the groups the surface
    misses; ``zscore`` (n, S): the marginal (Y - mean) / sqrt(var); ``pit`` (n,): mean_s Phi(zscore); ``keys`` (G,)."""
    *lgo, keys = lgoPredictive(g, groups, X_override, Y_override) if lgo is None else lgo
    elpd, groupwise, z, pit = _predictive_summary(g, Y_override, *lgo)
    return {"elpd": elpd, "groupwise": groupwise, "zscore": z, "pit": pit, "keys": keys}


def kfoldPredictive(g: GPSLCObject, K=None, seed=0, groups=None, X_override=None, Y_override=None):
    """K-fold cross-validation of the outcome model of every posterior sample (gpslc_y_kfold) -> ``(mean, var, lpd, keys)``, as
    ``lgoPredictive`` gives them, for groups of ANY size.  ``K``: the folds ``foldLabels(n, K, seed)`` (``keys`` = 0 .. K - 1);
    ``groups``: any length-n labelling (ints, strings); neither: the objects of the data (``g.obj``); both: ``ValueError``.  Groups of
    at most 128 members are computed exactly as ``lgoPredictive`` computes them (the same bits); larger ones through a tiled
    factorisation of their block of inv(A).  Overrides and errors as ``looPredictive``."""
    if K is not None and groups is not None:
        raise ValueError("kfoldPredictive takes K= (random folds) or groups= (a labelling), not both")
    keys, labels = _group_labels(g, foldLabels(g.getN(), K, seed) if K is not None else groups, "kfoldPredictive")
    ctx = g.ctx()
    st, mean, var, lpd, _ = ctx.y_kfold(g.getNumPosteriorSamples(), g.U, *_overrides(g, X_override, Y_override), g.uyLS, g.xyLS,
                                        g.tyLS, g.yScale, g.yNoise, len(keys), labels, want=("mean", "var", "lpd"))
    ctx.check(st)
    return mean, var, lpd, keys


def kfoldSummary(g: GPSLCObject, K=None, seed=0, groups=None, X_override=None, Y_override=None, kfold=None):
    """``lgoSummary``'s dictionary (``elpd``, ``groupwise``, ``zscore``, ``pit``, ``keys``) of ``kfoldPredictive`` (``kfold`` = its
    result, to summarise one already computed)."""
    *cv, keys = kfoldPredictive(g, K, seed, groups, X_override, Y_override) if kfold is None else kfold
    elpd, groupwise, z, pit = _predictive_summary(g, Y_override, *cv)
    return {"elpd": elpd, "groupwise": groupwise, "zscore": z, "pit": pit, "keys": keys}


# ------------------------------------------------------------------------------------------
# new individuals (no reference counterpart)
# ------------------------------------------------------------------------------------------

# What predictNew cannot be asked for, refused before any library call: (condition, exception, message), the first that fires.
# ``q.nX`` / ``q.nU``: the model's feature counts; ``q.X`` / ``q.like`` / ``q.U``: Xnew= / like= / Unew= given.
_NEW_REFUSALS = (
    (lambda q: q.fp32, ValueError, "predictNew needs an fp64 model: new individuals are not supported with fp32_kernel=True"),
    (lambda q: q.slope and q.base, ValueError,
     "slope=True cannot be combined with baseline=: the slope is a derivative at one level, not a contrast"),
    (lambda q: q.tnew and q.base, ValueError,
     "Tnew= cannot be combined with baseline=: Tnew is the baseline, each new individual's own treatment"),
    (lambda q: q.tnew and q.slope, ValueError,
     "Tnew= cannot be combined with slope=True: the slope is a derivative at one level, not a contrast"),
    (lambda q: q.slope and q.ndim == 2 and q.vec_ok, ValueError,
     "slope=True needs scalar levels: slopes at per-individual levels are not supported"),
    (lambda q: q.ndim > (2 if q.vec_ok else 1), ValueError,
     "{who} needs scalar levels{or_vec}: a new individual has no factual treatment unless Tnew= gives it; "
     "the ordinary effect f(a) - f(T) is the contrast with baseline = its treatment"),
    (lambda q: q.nX > 0 and not q.X, ValueError, "Xnew= is required: the model has nX = {nX} covariates"),
    (lambda q: q.nX == 0 and q.X, ValueError, "Xnew= cannot be given: the model has no covariates"),
    (lambda q: q.nU > 0 and q.like == q.U, ValueError,
     "exactly one of like= and Unew= is required: the model has nU = {nU} latent confounders, and a new individual's are the "
     "caller's to supply (like= copies a training individual's, a member of the same object)"),
    (lambda q: q.nU == 0 and (q.like or q.U), ValueError, "like= / Unew= cannot be given: the model has no latent confounders"),
)


def predictNew(g: GPSLCObject, doTs, Xnew=None, like=None, Unew=None, baseline=None, slope=False, want_var=True, want_cov=False,
               Tnew=None):
    """Predictions for m individuals who are not in the data (gpslc_predict_new) -> ``mean`` (m, S, L), ``var`` (m, S, L)
    [, ``cov`` (S, L, m, m) with ``want_cov=True``]: per posterior sample and level, the latent surface's value at the new
    covariates — the potential outcome f*(doT) by default, the contrast f*(doT) - f*(baseline) (the CATE at x*) with
    ``baseline=`` (a scalar or one value per level), the marginal effect d f*/dt at doT with ``slope=True`` — and its variance /
    joint covariance over the new individuals, + predictionCovarianceNoise as everywhere.  ``var`` is None with
    ``want_var=False``.

    ``Xnew`` (m, nX) is required iff the model has covariates.  With latent confounders exactly one of ``like`` (m training
    indices, 0-based: individual i takes U[like[i], :, s], a new member of a known object) and ``Unew`` (m, nU, S) is required.
    A model with neither has one kind of new individual: m = 1.

    Per-individual levels (gpslc_predict_new_vec): ``doTs`` may be an (L, m) array, level l setting new individual i to
    ``doTs[l, i]`` — a policy for a new population; ``baseline=`` may then be a scalar, (L,) or (L, m).  ``Tnew=`` (m,) gives
    the new individuals' own factual treatments and turns the call into the ordinary effect f*(a) - f*(Tnew_i), for scalar or
    per-individual ``doTs``; it excludes ``baseline=`` and ``slope=True``.  The value of a policy over the new population with
    its variance is ``w @ mean`` and ``w @ cov @ w`` on the host (``averageNew`` takes scalar levels only).  Refusals are raised
    before any library call; a failed factorisation raises ``PosDefException``."""
    levels, base, X, U, m, form, vec = _new_request(g, doTs, Xnew, like, Unew, baseline, slope, Tnew, who="predictNew")
    want = ("mean",) + (("var",) if want_var or want_cov else ()) + (("cov",) if want_cov else ())
    ctx = g.ctx()
    st, mean, var, cov = (ctx.predict_new_vec if vec else ctx.predict_new)(
        g.getNumPosteriorSamples(), g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, X, U, form, levels, base,
        g.hyperparams.predictionCovarianceNoise, want=want)
    ctx.check(st)
    var = var if want_var else None
    # (S, L, m, m) as a view of the library's m x m x S x L: every block is exactly symmetric, so no copy is needed to index it
    # [s, l, i, i']
    return (mean, var, np.transpose(cov, (2, 3, 0, 1))) if want_cov else (mean, var)


def _new_features(g, Xnew, like, Unew):
    """The new individuals' features as the library takes them -> (Xnew (m, nX) or None, Unew (m, nU, S) or None, m), column-major."""
    nX, nU, n, S = g.getNX(), g.getNU(), g.getN(), g.getNumPosteriorSamples()
    X = None
    if nX > 0:
        X = np.asarray(Xnew, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != nX or X.shape[0] < 1:
            raise ValueError(f"Xnew must be an (m, nX) array with nX = {nX}, got an array of shape {np.shape(Xnew)}")
        X = np.asfortranarray(X)
    U = None
    if like is not None:
        idx = np.asarray(like)
        if idx.ndim != 1 or idx.shape[0] < 1 or idx.dtype.kind not in "iu" or np.any(idx < 0) or np.any(idx >= n):
            raise ValueError(f"like must be a vector of training indices in 0..{n - 1}, one per new individual")
        U = np.take(g.U.T, idx, axis=2).T       # g.U[idx] column-major, gathered along the contiguous axis (10x faster than g.U[idx])
    elif Unew is not None:
        U = np.asarray(Unew, dtype=np.float64)
        if U.ndim != 3 or U.shape[1:] != (nU, S) or U.shape[0] < 1:
            raise ValueError(f"Unew must be an (m, nU, S) array with nU = {nU}, S = {S}, got an array of shape {np.shape(Unew)}")
        U = np.asfortranarray(U)
    m = X.shape[0] if X is not None else U.shape[0] if U is not None else 1
    if X is not None and U is not None and U.shape[0] != m:
        raise ValueError(f"Xnew has {m} rows but like / Unew names {U.shape[0]} new individuals")
    return X, U, m


def _new_request(g, doTs, Xnew, like, Unew, baseline, slope, Tnew=None, who=None):
    """The one plan of a call about new individuals, shared by predictNew and averageNew: the refusals of ``_NEW_REFUSALS`` and the
    parsing of the levels and of the new individuals' features -> (levels, base or None, Xnew (m, nX) or None, Unew (m, nU, S) or
    None, m, form, vec), the arrays column-major as the library takes them.  ``vec`` (predictNew alone, ``who`` given: a 2-D
    ``doTs`` or ``Tnew=``): levels and base are (m, L), per-individual; else (L,).  Raises before any library call."""
    nX, nU = g.getNX(), g.getNU()
    a = np.asarray(doTs, dtype=np.float64)
    q = SimpleNamespace(fp32=g.fp32_kernel, slope=bool(slope), base=baseline is not None, ndim=a.ndim, nX=nX, nU=nU,
                        X=Xnew is not None, like=like is not None, U=Unew is not None, tnew=Tnew is not None, vec_ok=who is not None)
    for cond, exc, msg in _NEW_REFUSALS:
        if cond(q):
            raise exc(msg.format(nX=nX, nU=nU, who=who or "averageNew", or_vec=" or an (L, m) array of per-individual levels" if who else ""))
    X, U, m = _new_features(g, Xnew, like, Unew)
    vec = a.ndim == 2 or Tnew is not None
    if a.ndim == 2 and a.shape[1] != m:
        raise ValueError(f"{who} needs scalar levels or an (L, m) array of per-individual levels with m = {m}, got an array of shape {a.shape}")
    if not vec:
        levels = np.ascontiguousarray(np.atleast_1d(a))
        base = None if baseline is None else _baseline(baseline, levels.shape[0])
    else:
        levels = np.asfortranarray(a.T if a.ndim == 2 else np.tile(np.atleast_1d(a)[None, :], (m, 1)))
        L, base = levels.shape[1], None
        if Tnew is not None:
            t = np.asarray(Tnew, dtype=np.float64)
            if t.shape != (m,):
                raise ValueError(f"Tnew must be a vector of m = {m} factual treatments, got an array of shape {t.shape}")
            base = np.asfortranarray(np.tile(t[:, None], (1, L)))
        elif baseline is not None:
            b = np.asarray(baseline, dtype=np.float64)
            if b.shape == (L, m):
                base = np.asfortranarray(b.T)
            elif b.ndim <= 1:
                base = np.asfortranarray(np.tile(_baseline(b, L)[None, :], (m, 1)))
            else:
                raise ValueError(f"baseline must be a scalar, one value per level (L = {L}) or an (L, m) array with m = {m}, "
                                 f"got an array of shape {b.shape}")
    for name, v in (("doTs", levels), ("Xnew", X), ("Unew", U), ("Tnew" if Tnew is not None else "baseline", base)):
        if v is not None and not np.all(np.isfinite(v)):
            raise ValueError(f"{name} has a non-finite entry")
    return levels, base, X, U, m, "slope" if slope else "outcome" if base is None else "contrast", vec


def testPredictive(g: GPSLCObject, Xtest=None, Ttest=None, Ytest=None, like=None, Utest=None):
    """The predictive distribution of a held-out test set under the outcome model of every posterior sample (gpslc_y_test) ->
    ``(mean, var, lpd, lpd_joint)``: ``mean``, ``var`` (m, S) of Ytest_i at the test individual's own treatment Ttest_i given
    the n training individuals (``var`` is for the observation: it includes yNoise), ``lpd`` (m, S) the log density of Ytest_i
    under it, ``lpd_joint`` (S,) the joint log density of the whole test set.  The chain has never seen the test set, so each
    sample's U and hyper-parameters were inferred without these outcomes: the clean out-of-sample comparison of models
    (nU = 0 / 1 / 2), which ``looPredictive`` / ``kfoldPredictive`` approximate on the training rows.  ``Xtest`` / ``like`` /
    ``Utest`` are ``predictNew``'s Xnew / like / Unew.  A failed factorisation raises ``PosDefException``."""
    if g.fp32_kernel:
        raise ValueError("testPredictive needs an fp64 model: new individuals are not supported with fp32_kernel=True")
    if Ttest is None or Ytest is None:
        raise ValueError("testPredictive needs Ttest= and Ytest=: the test set's treatments and outcomes")
    nX, nU = g.getNX(), g.getNU()
    q = SimpleNamespace(fp32=False, slope=False, base=False, ndim=1, nX=nX, nU=nU, X=Xtest is not None, like=like is not None,
                        U=Utest is not None, tnew=False, vec_ok=True)
    for cond, exc, msg in _NEW_REFUSALS:
        if cond(q):
            raise exc(msg.format(nX=nX, nU=nU, who="testPredictive", or_vec="").replace("Xnew", "Xtest").replace("Unew", "Utest"))
    X, U, m = _new_features(g, Xtest, like, Utest)
    T, Y = np.asarray(Ttest, dtype=np.float64), np.asarray(Ytest, dtype=np.float64)
    if m == 1 and X is None and U is None and T.ndim == 1:
        m = T.shape[0]      # a model with neither X nor U: the test set is its treatments and outcomes
    for name, v in (("Ttest", T), ("Ytest", Y)):
        if v.shape != (m,):
            raise ValueError(f"{name} must be a vector of m = {m} values, got an array of shape {v.shape}")
    for name, v in (("Xtest", X), ("Utest", U), ("Ttest", T), ("Ytest", Y)):
        if v is not None and not np.all(np.isfinite(v)):
            raise ValueError(f"{name} has a non-finite entry")
    ctx = g.ctx()
    st, mean, var, lpd, joint = ctx.y_test(g.getNumPosteriorSamples(), g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, X, U,
                                           np.ascontiguousarray(T), np.ascontiguousarray(Y))
    ctx.check(st)
    return mean, var, lpd, joint


def testSummary(g: GPSLCObject, Xtest=None, Ttest=None, Ytest=None, like=None, Utest=None, test=None):
    """Summaries of ``testPredictive`` (host arithmetic only; ``test`` = its result, to summarise one already computed):
    ``looSummary``'s ``elpd`` (S,), ``pointwise`` (m,), ``zscore`` (m, S) and ``pit`` (m,) of the test individuals, plus ``joint``
    (S,): the joint log density of the test set, and ``rmse`` (S,): sqrt(mean_i (Ytest_i - mean[i, s])^2)."""
    mean, var, lpd, joint = testPredictive(g, Xtest, Ttest, Ytest, like, Utest) if test is None else test
    Y = np.asarray(Ytest, dtype=np.float64)
    elpd, pointwise, z, pit = _predictive_summary(g, Y, mean, var, lpd, rows=Y.shape[0])
    return {"elpd": elpd, "pointwise": pointwise, "zscore": z, "pit": pit, "joint": joint,
            "rmse": np.sqrt(np.mean((Y[:, None] - mean) ** 2, axis=0))}


def averageNew(g: GPSLCObject, doTs, Xnew=None, like=None, Unew=None, weights=None, baseline=None, slope=False, want_cov=False):
    """Weighted averages over m individuals who are not in the data (gpslc_predict_new_weighted) -> ``mean`` (S, L[, G]), ``var``
    (S, L[, G]) [, ``cov`` (S, L, L[, G]) with ``want_cov=True``]: per posterior sample, level and weight column, the average
    tau_g = w_g' f* of what ``predictNew`` gives per individual — the outcome, the contrast with ``baseline=`` or the slope —
    over a target population that is not the sample, with the variance ``predictNew``'s ``var`` cannot give (the new individuals
    share one Gaussian process) and the joint covariance of the levels; no (m, m) array exists anywhere.

    ``weights=None`` is 1/m for everybody: the population average.  A length-m vector is one weight column (no group axis), an
    (G, m) array or a sequence of rows keeps it; Bool rows are group masks (the group's average), Float rows are used as given:
    a difference of two group rows is the difference of the groups with its correct variance; ``groupWeights(labels)`` builds
    the rows of a labelling of the new individuals.  ``Xnew`` / ``like`` / ``Unew`` / ``baseline`` / ``slope`` are
    ``predictNew``'s, parsed and refused as there.  The outputs have ``effectCurve``'s shapes: ``curveSamples(mean, cov, spp)``
    draws whole curves of the target population.  Levels are scalar: the value of a policy with per-individual doses over a new
    population, with its variance, is ``predictNew(..., want_cov=True)``'s ``cov`` contracted with the weights on the host
    (``w @ mean``, ``w @ cov @ w``).  A failed factorisation raises ``PosDefException``."""
    levels, base, X, U, m, form, _ = _new_request(g, doTs, Xnew, like, Unew, baseline, slope)
    W, is_vec = (np.full((1, m), 1.0 / m), True) if weights is None else _weights(weights, m)
    want = ("mean", "var") + (("cov",) if want_cov else ())
    ctx = g.ctx()
    st, mean, var, cov = ctx.predict_new_weighted(g.getNumPosteriorSamples(), g.U, g.uyLS, g.xyLS, g.tyLS, g.yScale, g.yNoise, m, X,
                                                  U, form, levels, base, W, g.hyperparams.predictionCovarianceNoise, want=want)
    ctx.check(st)
    out = (mean, var) + ((cov,) if want_cov else ())
    return tuple(o[..., 0] for o in out) if is_vec else out


def gpLogpdf(F, LS, scale, noise, target, ctx: Optional[Context] = None):
    """log N(target; 0, processCov(rbfKernelLog(F, F, LS), scale, noise)) on the GPU, for one parameter set
    (F (n, nF), LS (nF,), scalars) or S of them (F (n, nF, S) or shared (n, nF); LS (nF, S); scale, noise (S,);
    target (n, S) or shared (n,)): the :X => k => :X, :T / :logitT and :Y node scores of the reference's Gen
    models (src/model_likelihood.jl:13-120)."""
    scale = np.atleast_1d(np.asarray(scale, dtype=np.float64))
    noise = np.atleast_1d(np.asarray(noise, dtype=np.float64))
    S = scale.shape[0]
    target = _f(target)
    n = target.shape[0]
    t_shared = 1 if target.ndim == 1 else 0
    if F is None:
        nF, Fa, f_shared, ls = 0, None, 1, None
    else:
        Fa = _f(F)
        if Fa.ndim == 1:
            Fa = Fa[:, None]
        nF = Fa.shape[1]
        f_shared = 1 if Fa.ndim == 2 else 0
        ls = np.asfortranarray(np.asarray(LS, dtype=np.float64).reshape(nF, S, order="F"))
    own = ctx is None
    ctx = ctx or Context(n, 0, 0)
    if own:
        ctx.set_data(None, np.zeros(n), np.zeros(n))
    out = np.empty(S)
    st = ctx.lib.gpslc_gp_logpdf(ctx.h, S, nF, _p(Fa), f_shared, _p(ls), _p(scale), _p(noise), _p(target), t_shared,
                                 _p(out))
    ctx.check(st)
    return out


def _marshal_nodes(nodes, ctx):
    """gpslc_node array for a sequence of (F, LS, scale, noise, target); arrays shared by several nodes of the call (the
    same feature block under several parameter values, one target) are converted and addressed once."""
    cnt = len(nodes)
    arr = (_lib.Node * max(cnt, 1))()
    keep = []
    memo = {}

    def conv(a, shape=None):
        key = id(a)
        hit = memo.get(key)
        if hit is None:
            b = _f(a, shape)
            if b.ndim == 1 and shape is None:
                b = b[:, None]
            hit = memo[key] = (b, b.ctypes.data)
            keep.append(a)
        return hit

    for i, (F, LS, scale, noise, target) in enumerate(nodes):
        tg, tgp = conv(target, (ctx.n,))
        if F is None or (isinstance(F, np.ndarray) and F.size == 0) or (not isinstance(F, np.ndarray) and np.asarray(F).size == 0):
            Fp, lsp, nF = None, None, 0
        else:
            Fa, Fp = conv(F)
            nF = Fa.shape[1]
            ls = np.ascontiguousarray(LS, dtype=np.float64).reshape(nF)
            keep.append(ls)
            lsp = ls.ctypes.data
        nd = arr[i]
        nd.nF = nF
        nd.F = Fp
        nd.ls = lsp
        nd.scale = float(scale)
        nd.noise = float(noise)
        nd.target = tgp
    return arr, (keep, memo)


def nodesLogpdf(nodes, ctx: Context, fail_value=None):
    """The fused whole-model score (gpslc_nodes_logpdf): ``nodes`` is a sequence of (F, LS, scale, noise, target)
    — F (n, nF) or None, LS (nF,), scalars, target (n,) — one per Gen address to re-score (:X => k => :X, :T /
    :logitT, :Y with F = [U | X | T]; src/model_likelihood.jl:13-120).  One call, and for n <= 640 one kernel
    launch, whatever the nodes' feature counts.  Returns the log-densities (len(nodes),).
    A covariance that is not positive definite raises PosDefException (PDMats' behaviour inside Gen's mvnormal);
    with ``fail_value`` given, the failing nodes (gpslc_last_info) get that value instead and the others keep
    their scores — what a batch of independent MH proposals needs."""
    cnt = len(nodes)
    arr, _keep = _marshal_nodes(nodes, ctx)
    out = np.empty(cnt)
    st = ctx.lib.gpslc_nodes_logpdf(ctx.h, cnt, C.cast(arr, C.c_void_p), _p(out))
    if st > 0 and fail_value is not None:
        out[ctx.last_info(cnt) != 0] = fail_value
        return out
    ctx.check(st)
    return out


def nodesLogpdfGrad(nodes, ctx: Context, want=Context.NODE_GRAD_OUTPUTS):
    """The fused whole-model gradient (gpslc_nodes_logpdf_grad): ``nodes`` as for nodesLogpdf; one dict per
    node with ``dF`` (n, nF), ``dls`` (nF,), ``dscale``, ``dnoise``, ``dtarget`` (n,) and ``logpdf`` — the derivatives of the
    node's score with respect to its feature block, lengthscales, scale, noise and target (the parameters themselves, not
    their logarithms); outputs not named in ``want`` are None.  One call and, at the sizes the chains run at, one launch.
    A covariance that is not positive definite raises PosDefException."""
    st, out = ctx.nodes_logpdf_grad(nodes, want)
    ctx.check(st)
    res, fo, lo = [], 0, 0
    for i, nd in enumerate(nodes):
        F = nd[0]
        nF = 0 if F is None or np.size(F) == 0 else (1 if np.ndim(F) == 1 else np.shape(F)[1])
        res.append({"dF": None if out["dF"] is None else out["dF"][ctx.n * fo:ctx.n * (fo + nF)].reshape((ctx.n, nF), order="F"),
                    "dls": None if out["dls"] is None else out["dls"][lo:lo + nF],
                    "dscale": None if out["dscale"] is None else float(out["dscale"][i]),
                    "dnoise": None if out["dnoise"] is None else float(out["dnoise"][i]),
                    "dtarget": None if out["dtarget"] is None else out["dtarget"][:, i],
                    "logpdf": None if out["logpdf"] is None else float(out["logpdf"][i])})
        fo += nF
        lo += nF
    return res


def nodesDraw(nodes, ctx: Context):
    """Draws from the nodes' Gaussian priors (gpslc_nodes_draw): ``nodes`` as for nodesLogpdf, with standard normals z
    in the target slot; returns chol(K) z per node as the columns of an (n, len(nodes)) array — the `mvnormal(zeros(n),
    cov)` of an elliptical slice's auxiliary vector (src/inference.jl:225-232) or of a prior draw, with the
    random numbers still drawn on the host (any n: the single-workgroup kernels up to n = 640, the batched tiled
    factorisation + the predictive-draw kernel beyond)."""
    cnt = len(nodes)
    arr, _keep = _marshal_nodes(nodes, ctx)
    out = np.empty((ctx.n, cnt), order="F")
    ctx.check(ctx.lib.gpslc_nodes_draw(ctx.h, cnt, C.cast(arr, C.c_void_p), _p(out), None))
    return out


def mvnLogpdf(cov, x, covscale=None, ctx: Optional[Context] = None):
    """log N(x_s; 0, covscale_s * cov): the :U => u => :U node scores (uCov = SigmaU * uNoise,
    src/model_likelihood.jl:4-10, src/model_prior.jl:27-30).  ``cov=None`` re-uses the factor cached in
    ``ctx`` by an earlier call (SigmaU is constant for a data set)."""
    x = _f(x)
    if x.ndim == 1:
        x = x[:, None]
    n, S = x.shape
    covf = None
    if cov is not None:
        cov = np.asarray(cov, dtype=np.float64)
        covf = cov if cov.flags.f_contiguous or cov.flags.c_contiguous else np.ascontiguousarray(cov)  # symmetric
    cs = None if covscale is None else np.ascontiguousarray(np.atleast_1d(covscale), dtype=np.float64)
    ctx = ctx or Context(n, 0, 0)
    out = np.empty(S)
    st = ctx.lib.gpslc_mvn_logpdf(ctx.h, S, _p(covf), _p(cs), _p(x), _p(out))
    ctx.check(st)
    return out
