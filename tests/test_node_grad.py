"""The host restatement of a node's score gradient (node_grad_restatement.py) checked on itself, and the chain-rule assembly of
`_RealTChain.grad_xty` with the restatement in place of the library call: no GPU.

1. The long-double closed form against central differences (h = 1e-6) of a long-double log density, to 1e-9 of the scale: every
   feature column (not only a leading block), every lengthscale, scale, noise, target; the node without features too.
2. sum_r dF[r, f] vanishes to the bound (the score does not change when a column is shifted).
3. fp64 against long double: within 1e-3 of the bound the GPU tests use.
4. The inputs of the GPU tests (tests/test_gpu_node_grad.py) can see the two mistakes those tests are there to catch, on the
   single-launch kernel's 16 x 16 blocks (n = 17: one live row in a padded block; n = 150) and on the 128 x 128 tiles (n = 129):
   a padding that takes part moves dnoise and dscale, a missing transposed-block contribution moves dF, each by more than 1e6
   bounds.  The padding cannot move dF or dls: every extra term is an exact zero.
5. `grad_xty` is the gradient of `score_xty`'s sum: its dict against central differences of the summed restated scores over the
   traced U vectors and every hyper-parameter, on a real chain, a binary chain and a chain without covariates."""
import numpy as np
import pytest

import node_grad_restatement as ng

LD = np.longdouble
H = LD(1e-6)


def _fd(f):
    return (f(H) - f(-H)) / (2 * H)


@pytest.mark.parametrize("n,nF", [(24, 3), (40, 1), (17, 0)])
def test_closed_form_matches_central_differences(n, nF):
    F, ls, sc, nz, y = ng.random_node(n, nF, 3)
    g, s = ng.gradient((F, ls, sc, nz, y), LD)
    assert g["dF"].shape == (n, nF) and g["dls"].shape == (nF,)
    for f in range(nF):
        num = _fd(lambda e: ng.logpdf((F, ls.astype(LD) + e * np.eye(nF, dtype=LD)[f], sc, nz, y)))
        assert abs(num - g["dls"][f]) <= 1e-9 * s["dls"][f], ("ls", f, num, g["dls"][f])
        for i in range(0, n, 5):
            def moved(e):
                F2 = F.astype(LD)
                F2[i, f] += e
                return ng.logpdf((F2, ls, sc, nz, y))
            num = _fd(moved)
            assert abs(num - g["dF"][i, f]) <= 1e-9 * s["dF"][i, f], ("F", i, f, num, g["dF"][i, f])
    num = _fd(lambda e: ng.logpdf((F, ls, LD(sc) + e, nz, y)))
    assert abs(num - g["dscale"]) <= 1e-9 * s["dscale"], ("scale", num, g["dscale"])
    num = _fd(lambda e: ng.logpdf((F, ls, sc, LD(nz) + e, y)))
    assert abs(num - g["dnoise"]) <= 1e-9 * s["dnoise"], ("noise", num, g["dnoise"])
    for i in (2, n - 1):
        num = _fd(lambda e: ng.logpdf((F, ls, sc, nz, y.astype(LD) + e * np.eye(n, dtype=LD)[i])))
        assert abs(num - g["dtarget"][i]) <= 1e-9 * s["dtarget"][i], ("target", i, num, g["dtarget"][i])


@pytest.mark.parametrize("n,nF", [(17, 3), (150, 8), (129, 16)])
def test_fp64_restatement_and_shift_identity(n, nF):
    node = ng.random_node(n, nF, 1)
    gl, sl, tol, cond = ng.expected((n, nF, 1))
    g64, _ = ng.gradient(node, np.float64)
    err = ng.errors(g64, gl, sl)
    print("n", n, "nF", nF, "cond %.3g" % cond, "fp64 error / bound:", {k: v / tol for k, v in err.items()})
    assert max(err.values()) <= 1e-3 * tol, err
    assert np.all(np.abs(gl["dF"].sum(0)) <= tol * sl["dF"].sum(0))


@pytest.mark.parametrize("n,nF,block", [(17, 3, 16), (150, 8, 16), (129, 16, 128), (129, 32, 128)])
def test_the_inputs_can_see_a_missing_transposed_block_and_an_unmasked_padding(n, nF, block):
    node = ng.random_node(n, nF, 1)
    tol, _ = ng.node_tolerance(node)
    good, sc = ng.gradient(node)
    move = ng.errors(ng.gradient(node, block=block, no_transpose=True)[0], good, sc)
    print("without the blocks above the diagonal, in bounds:", {k: v / tol for k, v in move.items()})
    assert move["dF"] > 1e6 * tol
    move = ng.errors(ng.gradient(node, block=block, no_mask=True)[0], good, sc)
    print("with the padding taking part, in bounds:", {k: v / tol for k, v in move.items()})
    assert move["dnoise"] > 1e6 * tol and move["dscale"] > 1e6 * tol
    assert max(move["dF"], move["dls"]) <= 1e-3 * tol


# ---- grad_xty: the chain-rule assembly, with the restatement standing in for the library -------------------------------------

def _chain(binary, nU, nX, n=14, seed=5):
    """a `_RealTChain` with the state `_xty_nodes` reads and no context: nothing here touches the GPU"""
    from causalgpslc_jl_amd import inference as inf
    rng = np.random.default_rng(seed)
    ch = object.__new__(inf._RealTChain)
    ch.binary, ch.n, ch.nU, ch.nX, ch.ctx = binary, n, nU, nX, None
    ch.X = np.asfortranarray(rng.standard_normal((n, nX))) if nX else None
    ch.T = (rng.random(n) < 0.5).astype(np.float64) if binary else rng.standard_normal(n)
    ch.Y = rng.standard_normal(n)
    ch.logitT = rng.standard_normal(n) if binary else None
    u = lambda *shape: rng.uniform(1.2, 2.5, shape)     # noqa: E731
    v = {"yNoise": 0.4, "tyLS": 1.7, "yScale": 1.3}
    if nU or nX:
        v.update(tNoise=0.5, tScale=0.9)
    if nU:
        v.update(utLS=u(nU), uyLS=u(nU))
    if nX:
        v.update(xtLS=u(nX), xyLS=u(nX))
    if nU and nX:
        v.update(uxLS=u(nU, nX), xNoise=rng.uniform(0.3, 0.8, nX), xScale=rng.uniform(0.8, 1.5, nX))
    ch.v = v
    ch.U = [rng.standard_normal(n) for _ in range(nU)]
    return ch


def _restated(nodes, ctx, want=None):
    out = []
    for nd in nodes:
        g, _ = ng.gradient(nd, LD)
        out.append({k: (float(g[k]) if np.ndim(g[k]) == 0 else np.asarray(g[k], dtype=np.float64)) for k in ng.OUTPUTS})
    return out


def _total(ch, v, U):
    nodes, _, _ = ch._xty_nodes(v, U)
    return sum(ng.logpdf(nd) for nd in nodes)


@pytest.mark.parametrize("binary,nU,nX", [(False, 2, 3), (True, 2, 3), (False, 2, 0), (True, 0, 2)])
def test_grad_xty_is_the_gradient_of_the_summed_scores(monkeypatch, binary, nU, nX):
    from causalgpslc_jl_amd import inference as inf
    ch = _chain(binary, nU, nX)
    monkeypatch.setattr(inf.api, "nodesLogpdfGrad", _restated)
    g = ch.grad_xty(U=ch.U)
    has_t = bool(nU or nX)
    names = {"tyLS", "yScale", "yNoise"} | ({"tScale", "tNoise"} if has_t else set()) | ({"dlogitT"} if binary and has_t else set())
    names |= ({"dU", "dUm", "utLS", "uyLS"} if nU else set()) | ({"xtLS", "xyLS"} if nX else set())
    names |= {"uxLS", "xScale", "xNoise"} if nU and nX else set()
    assert set(g) == names
    scale = max(1.0, *(float(np.max(np.abs(x))) for x in g.values() if np.size(x)))
    tol = 1e-8 * scale          # central differences of a long-double sum at h = 1e-6: h^2 times a third derivative of order one

    def moved(name, idx, e):
        v = {k: (np.array(x, dtype=LD) if isinstance(x, np.ndarray) else x) for k, x in ch.v.items()}
        if idx is None:
            v[name] = LD(v[name]) + e
        else:
            v[name][idx] += e
        return _total(ch, v, ch.U)

    for name in sorted(names - {"dU", "dUm", "dlogitT"}):
        cur = ch.v[name]
        for idx in ([None] if np.ndim(cur) == 0 else list(np.ndindex(np.shape(cur)))):
            num = _fd(lambda e: moved(name, idx, e))
            got = g[name] if idx is None else g[name][idx]
            assert abs(num - got) <= tol, (name, idx, float(num), got)
    for u in range(nU):
        assert g["dU"][u].shape == (ch.n,)
        for i in (0, 5, ch.n - 1):
            def moved_u(e):
                U = [np.array(x, dtype=LD) for x in ch.U]
                U[u][i] += e
                return _total(ch, ch.v, U)
            num = _fd(moved_u)
            assert abs(num - g["dU"][u][i]) <= tol, ("U", u, i, float(num), g["dU"][u][i])
    if nU:      # dUm is the same numbers in the model-side layout
        assert np.array_equal(inf.toMatrixModel(g["dU"], ch.n, nU), g["dUm"])
    if binary and has_t:
        for i in (1, ch.n - 2):
            def moved_l(e):
                keep = ch.logitT
                ch.logitT = keep.astype(LD) + e * np.eye(ch.n, dtype=LD)[i]
                try:
                    return _total(ch, ch.v, ch.U)
                finally:
                    ch.logitT = keep
            num = _fd(moved_l)
            assert abs(num - g["dlogitT"][i]) <= tol, ("logitT", i, float(num), g["dlogitT"][i])
