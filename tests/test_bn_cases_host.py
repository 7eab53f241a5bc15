"""Runs every case builder of tests/bn_cases.py on the CPU and asserts, from the float64 reference alone, that each case is in the regime it is named for, that no
entry lies inside a decision margin, that the planted ties are ties, that the plain fp32 evaluation stays below 1e-6 on every output (the rule of
tests/test_bn_kernels_gpu.py is then a bound of a few 1e-6 at the most), and — through the library's workspace queries — that the shape tables reach every geometry
and chunking class of the kernels.  No GPU."""
import math

import pytest
import torch

import bn_cases as BC

E_PLAIN = 1e-6


def _lib():
    from keypointfusion_amd import lib as L
    return L.load()


def _sound(case, skip=()):
    """Finite, of the right precision, and well conditioned: e_plain < 1e-6 for every output (an output that is exactly 0 in float64 is exactly 0 in fp32)."""
    for k, ref in case["ref"].items():
        plain = case["plain"][k]
        assert ref.dtype == torch.float64 and plain.dtype == torch.float32 and ref.shape == plain.shape, k
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(plain).all()), k
        if float(ref.abs().max()) == 0:
            assert float(plain.abs().max()) == 0, k
        elif k not in skip:
            assert BC.rel_err(plain, ref) < E_PLAIN, (k, BC.rel_err(plain, ref))


def _z(x):
    x = x.double()
    return (x - x.mean(0)) / x.std(0, unbiased=False)


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn_train_*
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,regime", BC.TRAIN_CASES)
def test_train_case(M, C, regime):
    c = BC.train_case(M, C, regime)
    _sound(c)
    x, ref, pl = c["x"], c["ref"], c["planted"]
    x64 = x.double()
    assert (pl is None) == (regime == "ordinary")
    # the relu'd backward is given y: its mask is the float64 forward's
    assert bool(torch.equal(c["y_in"] > 0, ref["pre"] > 0)) and bool(torch.equal(c["mask"], ref["pre"] > 0))
    if M >= 37:
        assert 0.2 < float(c["mask"].double().mean()) < 0.8
        db = ref["db0"].abs() / math.sqrt(M)
        assert float(db[1::2].median()) > 3 and float(db[0::2].median()) < 1.5  # db of the odd channels is not a pure cancellation
    if M == 1:
        assert float((ref["invstd"] * math.sqrt(BC.EPS) - 1).abs().max()) < 1e-12 and float((ref["y0"][0] - c["b"].double()).abs().max()) < 1e-12
        assert bool(torch.equal(ref["rvar"], c["rv"].double() * (1 - BC.MOMENTUM)))  # the batch variance of one row enters as 0: no n / (n - 1)
    if regime == "ordinary" and M > 2:
        z0 = _z(x)[0].abs()
        assert float(z0.max()) < 6
    if regime == "offset":
        mean, std = x64.mean(0), x64.std(0, unbiased=False)
        assert bool(((mean.abs() / std - BC.OFFSET_SIGMAS).abs() < 0.1 * BC.OFFSET_SIGMAS).all()) and bool((mean > 0).any()) and bool((mean < 0).any())
        assert bool(torch.equal(mean.float().double(), mean))  # the mean is an fp32 number
        assert float((x64 ** 2).mean(0).div(std ** 2).min()) > 5e5  # what a sum of squares about 0 would have to cancel
    if regime == "outlier":
        rows = c["outlier_rows"]
        S, rpc = BC.bn_chunks(M, C)
        assert rows == [0, rpc] and S > 1 and pl == list(range(0, C, 4))
        rest = torch.ones(M, dtype=torch.bool)
        rest[rows] = False
        zr = (x64[rows] - x64[rest].mean(0)) / x64[rest].std(0, unbiased=False)
        assert bool(((zr[:, pl].abs() - BC.OUTLIER_Z).abs() < 1e-3).all()) and bool((zr[:, pl] > 0).any()) and bool((zr[:, pl] < 0).any())
        z = _z(x)
        assert float(z[rows][:, pl].abs().min()) > 12  # (in its own channel's statistics, which the two outliers widen)
        others = [i for i in range(C) if i % 4]
        assert float(z[rows][:, others].abs().max()) < 6
    if regime == "constant":
        assert pl == [1, C - 2]
        for ch in pl:
            assert bool((x[:, ch] == x[0, ch]).all())
            assert abs(float(ref["invstd"][ch]) * math.sqrt(BC.EPS) - 1) < 1e-12 and float(ref["mean"][ch]) == float(x[0, ch])
            assert float((ref["y0"][:, ch] - c["b"][ch].double()).abs().max()) < 1e-12
            assert abs(float(ref["dw0"][ch])) < 1e-9 and float(ref["dx0"][:, ch].abs().max()) > 10 * float(ref["dx0"][:, 0].abs().max())  # finite and large: w / sqrt(eps)
        assert float(x64.std(0)[[i for i in range(C) if i not in pl]].min()) > 0.3
    if regime == "tiny":
        std = x64.std(0, unbiased=False)
        assert 0.4 * BC.TINY_SIGMA < float(std.min()) and float(std.max()) < 2.2 * BC.TINY_SIGMA
        assert float((std ** 2).max()) < 0.01 * BC.EPS and float(ref["invstd"].min()) > 0.99 / math.sqrt(BC.EPS)
    if regime == "negw":
        w = c["w"]
        assert bool((w[pl] <= 0).all()) and int((w == 0).sum()) >= 2 and int((w < 0).sum()) >= 2 and bool((w[[i for i in range(C) if i not in pl]] > 0).all())
        zero = (w == 0).nonzero().flatten()
        assert float(ref["dx0"][:, zero].abs().max()) == 0 and float(ref["dw0"][zero].abs().min()) > 0
    else:
        assert bool((c["w"] > 0).all())


@pytest.mark.parametrize("xdt,ydt", BC.H16_PAIRS)
@pytest.mark.parametrize("M,C", BC.H16_SHAPES)
def test_train_h16_case(M, C, xdt, ydt):
    c = BC.train_h16_case(M, C, xdt, ydt)
    _sound(c)
    assert c["x"].dtype == c["addend"].dtype == BC.TORCH_DT[xdt] and c["dy"].dtype == c["y_in"].dtype == BC.TORCH_DT[ydt]
    assert bool(torch.equal(c["mask"], c["y_in"].float() > 0))
    flipped = float((c["mask"] != (c["ref"]["pre"] > 0)).double().mean())  # positive values that round to 0 in the stored y
    assert flipped < 1e-3, flipped


def test_shape_table_reaches_every_class_of_the_statistics_kernels():
    lib = _lib()
    geo = {}
    for M, C in BC.SHAPES:
        ws = lib.kpf_bn_ws_floats(M, C)
        assert (ws - 2 * C) % (2 * C) == 0
        S, rpc = BC.bn_chunks(M, C)
        assert (ws - 2 * C) // (2 * C) == S and (S - 1) * rpc < M <= S * rpc, (M, C)
        assert lib.kpf_bn2_ws_floats(M, C) == 2 * ws
        Q, QL, RL, cg = BC.bn_geom(C)
        geo[(M, C)] = dict(S=S, rpc=rpc, Q=Q, QL=QL, RL=RL, cg=cg, last=M - (S - 1) * rpc, smax=(M + 4 * RL - 1) // (4 * RL))
    v = list(geo.values())
    assert any(256 % g["Q"] for g in v if g["Q"] < 64), "a quad count that does not divide 256: idle threads"
    assert any(g["Q"] == 64 for g in v)
    assert any(g["cg"] == 3 and g["Q"] % 64 == 16 for g in v) and any(g["cg"] == 2 and g["Q"] % 64 == 1 for g in v), "a partial last column group"
    # the finalize: wave g of 16 takes chunks g, g + 16, ...; four chains while g + 48 < S, then one
    assert any(g["S"] == 1 for g in v) and any(1 < g["S"] < 16 for g in v), "S below the 16 waves"
    assert any(g["S"] == 64 for g in v), "the 4-chain loop exactly once for every wave, no tail"
    assert any(g["S"] > 64 and g["S"] % 64 for g in v), "the 4-chain loop and its tail"
    assert any(g["smax"] > BC.BN_TARGET // g["cg"] and g["last"] < g["rpc"] for g in v), "the cap on S, a short last chunk"
    assert any(M == 1 for M, _ in geo) and any(M == 2 for M, _ in geo)
    assert any(g["S"] == 1 and M <= g["RL"] for (M, _), g in geo.items() if M > 1), "no thread with more than one row"
    assert any(g["S"] > 1 and g["last"] < g["RL"] for g in v), "a thread without rows in a chunk that has some"
    for M, C in BC.REGIME_SHAPES + BC.H16_SHAPES + BC.BN2_SHAPES:
        assert (M, C) in geo
    assert {r for _, _, r in BC.TRAIN_CASES} == set(BC.REGIMES) and all((M, C, r) in BC.TRAIN_CASES for M, C in BC.REGIME_SHAPES for r in BC.REGIMES)
    assert len(BC.REGIME_SHAPES) >= 2 and len(set(BC.H16_PAIRS)) == 5


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn2_add_relu_*
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", BC.BN2_SHAPES)
def test_bn2_case(M, C):
    c = BC.bn2_case(M, C)
    _sound(c)
    pre = c["ref"]["pre"]
    assert not bool((pre.abs() < BC.MARGIN * pre.abs().max()).any())  # the kernel's out > 0 cannot come out otherwise
    assert bool(torch.equal(c["mask"], pre > 0)) and bool(torch.equal(c["out_in"] > 0, pre > 0))
    assert bool((c["wb"] < 0).any()) and bool((c["wa"] > 0).all())
    if M >= 37:
        assert 0.2 < float(c["mask"].double().mean()) < 0.8


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn_relu_gmax_*
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,group,C,ld", BC.GMAX_SHAPES)
def test_gmax_case(G, group, C, ld):
    c = BC.gmax_case(G, group, C, ld)
    _sound(c)
    ref, arg, x = c["ref"], c["arg"].long(), c["x"].view(G, group, C)
    pre = ref["pre"]
    assert float(BC.gmax_margins(pre, G, group).min()) >= BC.MARGIN * float(pre.abs().max())
    z = torch.relu(pre).view(G, group, C)
    assert bool(torch.equal(arg, BC.first_argmax(z))) and bool(torch.equal(torch.gather(z, 1, arg.unsqueeze(1)).squeeze(1), ref["y"]))
    assert bool(torch.equal(c["mask"], ref["y"] > 0)) and bool(torch.equal(c["y_in"] > 0, ref["y"] > 0))
    neg = c["neg"]
    assert bool(neg.any()) and bool((c["w"][neg] < 0).all()) and bool((c["w"][~neg] > 0).all())
    won = torch.gather(x, 1, arg.unsqueeze(1)).squeeze(1)
    live = ref["y"] > 0
    assert bool((won == torch.where(neg, x.amin(1), x.amax(1)))[live].all())  # a negative scale: the winner has the smallest x
    if group > 1:
        m1, m2 = c["m1"], c["m2"]
        assert m1 < m2 and bool(torch.equal(x[0, m1], x[0, m2])) and bool((arg[0] == m1).all()) and bool((ref["y"][0] > 0).all())
        assert bool((z[0, m1] == z[0, m2]).all())  # an exact tie: the first member wins
        assert bool((pre.view(G, group, C)[1] < 0).all()) and bool((arg[1] == 0).all()) and bool((ref["y"][1] == 0).all())  # a group without a positive member
        assert float(ref["dx"].view(G, group, C)[1].abs().max()) > 0  # (its rows still receive the batch terms of dx)
    else:
        assert bool((arg == 0).all())
    assert int(arg.max()) == (group - 1 if group > 1 else 0) or group == 256
    assert 0.2 < float(live.double().mean()) < 1.0  # (group = 1 with every b below -0.2: a quarter of the entries)


def test_gmax_table_reaches_every_class():
    lib = _lib()
    assert {g for _, g, _, _ in BC.GMAX_SHAPES} == {1, 7, 64, 256}
    assert any(ld > C for *_, C, ld in BC.GMAX_SHAPES) and any(ld == C for *_, C, ld in BC.GMAX_SHAPES)
    chunks = {G: BC.gmax_bwd_chunks(G) for G, *_ in BC.GMAX_SHAPES}
    assert any(G < 64 and S == G for G, (S, _) in chunks.items()) and any(G > 64 and gpc > 1 and S * gpc > G for G, (S, gpc) in chunks.items())
    assert any(C % 256 for *_, C, _ in BC.GMAX_SHAPES if C > 256) and any(C < 16 for *_, C, _ in BC.GMAX_SHAPES)
    for G, group, C, _ in BC.GMAX_SHAPES:
        S = BC.bn_chunks(G * group, C)[0]
        assert lib.kpf_bn_relu_gmax_ws_floats(G * group, C) == max(S, 64) * 2 * C + 2 * C


# ----------------------------------------------------------------------------------------------------------------------------------------
# kpf_bn_ssr_*
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,n1,n2", BC.SSR_SHAPES)
def test_ssr_case(rows, C, n1, n2):
    c = BC.ssr_case(rows, C, n1, n2)
    _sound(c)
    s1, pre = c["ref"]["s1"], c["ref"]["pre"]
    assert not bool((s1.abs() < BC.MARGIN * s1.abs().max()).any()) and not bool((pre.abs() < BC.MARGIN * pre.abs().max()).any())
    assert bool(torch.equal(c["masks"][0], pre > 0)) and bool(torch.equal(c["out_in"] > 0, pre > 0)) and bool(torch.equal(c["masks"][1], s1 > 0))
    assert 0.1 < float(c["masks"][0].double().mean()) < 0.9 and 0.1 < float(c["masks"][1].double().mean()) < 0.9
    if n2:
        assert bool((c["masks"][0] & ~c["masks"][1]).any()) and bool((~c["masks"][0] & c["masks"][1]).any())  # the two masks are not one
    assert bool((c["w"] < 0).any())


def test_ssr_table_reaches_every_class():
    lib = _lib()
    sh = BC.SSR_SHAPES
    assert {(4096, 128, 3, 1), (672, 128, 2, 0), (77, 24, 1, 2), (33, 8, 4, 0)} <= set(sh)
    assert any(C == 256 for _, C, _, _ in sh) and any(n1 + n2 == 4 and n2 > 0 for _, _, n1, n2 in sh) and any(n1 + n2 == 4 and n2 == 0 for _, _, n1, n2 in sh)
    assert any(256 % (C // 4) for _, C, _, _ in sh), "idle threads in the backward's sums"
    for rows, C, n1, n2 in sh:
        n = n1 + n2
        S1, S2 = BC.bn_chunks(rows, n * C)[0], BC.ssr_chunks(rows, C // 4)[0]
        assert lib.kpf_bn_ssr_ws_floats(rows, C, n) == max(S1, S2) * 2 * n * C + 2 * n * C
    assert any(BC.ssr_chunks(rows, C // 4)[0] > BC.bn_chunks(rows, (n1 + n2) * C)[0] for rows, C, n1, n2 in sh)
    assert any(BC.bn_geom((n1 + n2) * C)[3] > 1 for _, C, n1, n2 in sh), "more than one column group in the statistics pass"
