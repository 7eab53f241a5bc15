"""Seeded cases for the train-mode BatchNorm kernels (csrc/kpf_wgrad.hip, section 3): kpf_bn_train_*, kpf_bn2_add_relu_*, kpf_bn_relu_gmax_*, kpf_bn_ssr_*.  For
each entry point: inputs as fp32 CPU tensors, the float64 restatement (torch.batch_norm in training mode plus relu / add / group maximum / slice sums, differentiated
with autograd), the same restatement in plain fp32 on the CPU, and what was planted where.  No GPU is touched here.

Every builder is cached (functools.lru_cache): tests/test_bn_cases_host.py asserts the regime of each case from the reference alone, and
tests/test_bn_kernels_gpu.py holds the kernels to  e_kernel <= 4 * e_plain + 8 * 2^-24  on the same objects, which no test modifies.

Decisions.  A backward entry point is given y / out / arg, mean and invstd as the float64 reference rounded to fp32, never a forward kernel's output, and both
restatements differentiate with the decisions of the float64 forward (ReLU masks, winners) held fixed: the plain fp32 evaluation then differs from the reference by
rounding alone, and so must the kernel.  Where a kernel decides in fp32 what the reference decided in float64 — `S1 > 0` of kpf_bn_ssr_*, `out > 0` of
kpf_bn2_add_relu_*, the winner of kpf_bn_relu_gmax_forward — the builder draws again every entry whose float64 margin is below MARGIN * max|pre-activation|, until
none is left.

A case is a dict:  inputs by name,  "ref" (float64) and "plain" (fp32) results by output name,  "planted": the planted channels (None: nothing planted)."""
import functools

import torch

from train_head_cases import FLOOR, SLICE_FLOOR, _gen, rel_err  # noqa: F401  (the rule's two constants and its error measure: one definition)

EPS = 1e-5
MOMENTUM = 0.1
MARGIN = 64 * 2.0 ** -24
BN_TARGET = 1024  # workgroups the chunking of the statistics pass aims at (bn_chunks)


# ----------------------------------------------------------------------------------------------------------------------------------------
# geometry: a restatement of bn_geom / bn_chunks / ssr_chunks and of the gmax backward's chunks (the host test holds it to the workspace queries)
# ----------------------------------------------------------------------------------------------------------------------------------------
def bn_geom(C):
    """-> (Q channel quads, QL quads per workgroup row, RL row lanes, cg column groups of 64 quads)."""
    Q = C // 4
    QL = min(Q, 64)
    return Q, QL, 256 // QL, (Q + 63) // 64


def bn_chunks(M, C):
    """-> (S chunks, rows per chunk): at least four rows per thread, at most BN_TARGET / cg chunks."""
    Q, QL, RL, cg = bn_geom(C)
    S = max(1, min(BN_TARGET // cg, (M + 4 * RL - 1) // (4 * RL)))
    rpc = (M + S - 1) // S
    return (M + rpc - 1) // rpc, rpc


def ssr_chunks(rows, C4):
    RL = 256 // C4
    S = max(1, min(1024, (rows + 2 * RL - 1) // (2 * RL)))
    rpc = (rows + S - 1) // S
    return (rows + rpc - 1) // rpc, rpc


def gmax_bwd_chunks(G):
    S = min(G, 64)
    gpc = (G + S - 1) // S
    return (G + gpc - 1) // gpc, gpc


# ----------------------------------------------------------------------------------------------------------------------------------------
# the restatement's pieces
# ----------------------------------------------------------------------------------------------------------------------------------------
def _bn(x, w, b, rm, rv):
    """Train-mode batch norm of rows [M][C]; rm / rv (None or tensors of x's precision) are updated in place.  M = 1: the batch variance is 0 and the running
    variance takes it as it is (there is no unbiased estimate of one row).
    float64: torch.batch_norm.  fp32: the operation written out in fp32 tensors, (x - mean) * (w / sqrt(mean((x - mean)^2) + eps)) + b, about the batch mean
    rounded ONCE to fp32 (`_mean32`).  ATen's own fp32 kernel on the CPU is not used: its batch mean is up to 14 ulp off (a constant channel of 1.7 comes out as
    1.699998) and it evaluates x * alpha + (b - mean * alpha), which cancels where |mean| >> sigma; either would widen the rule by two to three digits for a
    reason that is not in the operation."""
    M = x.shape[0]
    if x.dtype == torch.float64:
        if M > 1 or rm is None:
            return torch.batch_norm(x, w, b, rm, rv, True, MOMENTUM, EPS, False)
        y = torch.batch_norm(x, w, b, None, None, True, MOMENTUM, EPS, False)
        mean, var = x.detach()[0], torch.zeros_like(x[0])
    else:
        mean = x.mean(0)
        mean = mean + (_mean32(x) - mean).detach()  # the value of _mean32, the gradient of the mean
        xc = x - mean
        var = (xc * xc).mean(0)
        y = xc * (w / torch.sqrt(var + EPS)) + b
    if rm is not None:
        with torch.no_grad():
            rm.mul_(1 - MOMENTUM).add_(MOMENTUM * mean)
            rv.mul_(1 - MOMENTUM).add_(MOMENTUM * var * (M / (M - 1.0) if M > 1 else 1.0))
    return y


def _mean32(x):
    """The batch mean of fp32 rows as well as fp32 can hold it: summed in float64, rounded once."""
    return x.detach().double().mean(0).float()


def _stats(x):
    """-> (batch mean, 1 / sqrt(biased variance + eps)) in x's precision."""
    if x.dtype == torch.float32:
        mean = _mean32(x)
        return mean, 1 / torch.sqrt(((x - mean) ** 2).mean(0) + EPS)
    return x.mean(0), 1 / torch.sqrt(x.var(0, unbiased=False) + EPS)


def _leaves(t, *vs):
    return [t(v).detach().clone().requires_grad_(True) for v in vs]


def _dy(g, rows, C):
    """An incoming gradient with a per-channel offset of +-4 / sqrt(rows) in the odd channels: db lies four of its standard deviations from 0 there, not a pure
    cancellation.  (No larger: the backward is given the batch mean in fp32, and dw = sum dz (x - mean) invstd picks up db times that rounding.)"""
    c = torch.arange(C)
    return torch.randn(rows, C, generator=g) + torch.where(c % 2 == 1, 4.0 * rows ** -0.5 * (1.0 - 2.0 * ((c // 2) % 2)), torch.zeros(()))


def _params(g, C):
    return 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)  # w, b, rm, rv


def _rows(g, M, C):
    """Ordinary rows: per-channel sigma in [0.5, 2], per-channel mean of a few sigma."""
    sig, mu = 0.5 + 1.5 * torch.rand(C, generator=g), 2.0 * torch.randn(C, generator=g)
    return torch.randn(M, C, generator=g) * sig + mu, sig, mu


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. kpf_bn_train_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
# (M, C): the smallest shapes that reach each geometry and chunking class (tests/test_bn_cases_host.py proves it through kpf_bn_ws_floats)
SHAPES = [(1, 8),        # variance 0, the M > 1 guard of the running variance
          (2, 4),
          (37, 8),       # RL = 128: no thread has more than one row
          (777, 48),     # Q = 12 does not divide 256: four idle threads; S = 10 < 16 waves of the finalize
          (1024, 256),   # S = 64: the 4-chain loop of the finalize exactly once, no tail
          (1603, 256),   # exactly 64 quads; S = 101: the 4-chain loop and its tail; a last chunk of 3 rows for 4 row lanes
          (515, 576),    # three column groups, the last with 16 quads
          (300, 260),    # a second column group of one quad
          (16400, 256)]  # the cap on S (BN_TARGET), a short last chunk
REGIMES = ["ordinary", "offset", "outlier", "constant", "tiny", "negw"]
REGIME_SHAPES = [(777, 48), (1603, 256)]
TRAIN_CASES = [(M, C, "ordinary") for M, C in SHAPES] + [(M, C, r) for M, C in REGIME_SHAPES for r in REGIMES[1:]]
OUTLIER_Z = 30.0
OFFSET_SIGMAS = 1000.0
TINY_SIGMA = 1e-4


@functools.lru_cache(maxsize=None)
def train_input(M, C, regime):
    """x [M][C], w, b, running statistics, dy, addend and the planted channels of a regime:
      ordinary  sigma in [0.5, 2], mean of a few sigma;
      offset    every channel's mean is +-1000 sigma.  The rows lie on a lattice of sigma / 64 (sigma a power of two) and sum to M * offset exactly, so the
                channel mean is an fp32 number: the comparison judges the variance (a sum of squares about 0 loses six digits here), not the rounding of a
                mean that no fp32 kernel can store;
      outlier   in every fourth channel row 0 and the first row of the second chunk lie at +-30 standard deviations of the other rows from their mean;
      constant  channels 1 and C - 2 are exactly constant: variance 0, invstd = 1 / sqrt(eps), a finite backward;
      tiny      sigma = 1e-4 in every channel against eps = 1e-5: eps dominates invstd;
      negw      w negative in every third channel and zero in channels 1, 6, 11, ..."""
    g = _gen(M, C, REGIMES.index(regime), 31)
    x, sig, mu = _rows(g, M, C)
    w, b, rm, rv = _params(g, C)
    planted, rows = None, []
    if regime == "offset":
        sig = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
        n = torch.round(64 * torch.randn(M, C, generator=g, dtype=torch.float64))
        n -= torch.round(n.sum(0) / M)
        res = n.sum(0)  # |res| <= M / 2: taken off one unit per row
        n -= torch.sign(res) * (torch.arange(M, dtype=torch.float64).unsqueeze(1) < res.abs())
        assert bool((n.sum(0) == 0).all())
        sign = 1.0 - 2.0 * (torch.arange(C) % 2)
        x = ((n + 64 * OFFSET_SIGMAS * sign) * (sig.double() / 64)).float()
        planted = list(range(C))
    elif regime == "outlier":
        planted = list(range(0, C, 4))
        S, rpc = bn_chunks(M, C)
        rows = [0, rpc] if S > 1 else [0]
        rest = torch.ones(M, dtype=torch.bool)
        rest[rows] = False
        m_rest, s_rest = x[rest].double().mean(0), x[rest].double().std(0, unbiased=False)
        sign = 1.0 - 2.0 * ((torch.arange(C) // 4) % 2)
        for r in rows:
            x[r, planted] = (m_rest + OUTLIER_Z * sign * s_rest).float()[planted]
    elif regime == "constant":
        planted = [1, C - 2]
        x[:, 1], x[:, C - 2] = 1.7, -0.3
    elif regime == "tiny":
        x = x * TINY_SIGMA
        planted = list(range(C))
    elif regime == "negw":
        c = torch.arange(C)
        w = torch.where(c % 3 == 0, -w, w)
        w[c % 5 == 1] = 0.0
        planted = [i for i in range(C) if i % 3 == 0 or i % 5 == 1]
    else:
        assert regime == "ordinary"
        if M == 2:  # two rows sqrt(eps) apart: with a spread >> sqrt(eps) the normalised rows are +-1 and dx is the difference of two equal numbers
            x = 3e-3 * torch.randn(M, C, generator=g)
    dy = _dy(g, M, C)
    addend = torch.randn(M, C, generator=g)
    return dict(x=x.contiguous(), w=w, b=b, rm=rm, rv=rv, dy=dy, addend=addend, planted=planted, outlier_rows=rows, sigma=sig)


def _train_restate(t, x, w, b, rm, rv, dy, mask):
    """-> outputs by name; `mask` (y > 0 as the backward is given it; None: differentiate relu itself) is held fixed in the relu'd backward."""
    out = {}
    for relu in (0, 1):
        xl, wl, bl = _leaves(t, x, w, b)
        r1, r2 = t(rm).clone(), t(rv).clone()
        pre = _bn(xl, wl, bl, r1, r2)
        y = torch.relu(pre) if relu else pre
        fixed = pre * t(mask) if relu and mask is not None else y
        (fixed * t(dy)).sum().backward()
        out.update({"y%d" % relu: y.detach(), "dx%d" % relu: xl.grad, "dw%d" % relu: wl.grad, "db%d" % relu: bl.grad})
        out["rmean"], out["rvar"] = r1, r2
    out["pre"] = out["y0"]
    out["mean"], out["invstd"] = _stats(t(x))
    return out


def _train_refs(x, w, b, rm, rv, dy, addend, mask=None):
    d64, d32 = lambda v: v.double(), lambda v: v.float()
    ref = _train_restate(d64, x, w, b, rm, rv, dy, mask)
    if mask is None:
        mask = ref["y1"].float() > 0
    plain = _train_restate(d32, x, w, b, rm, rv, dy, mask)
    for side, t in ((ref, d64), (plain, d32)):
        for relu in (0, 1):
            side["dxa%d" % relu] = side["dx%d" % relu] + t(addend)
    return ref, plain, mask


@functools.lru_cache(maxsize=None)
def train_case(M, C, regime):
    """ref / plain: y0, y1 (relu off / on), mean, invstd, rmean, rvar, dx*, dxa* (with the addend), dw*, db*.  The backward's inputs: y_in (the reference's relu'd
    output in fp32), mean_in, invstd_in."""
    c = dict(train_input(M, C, regime))
    ref, plain, mask = _train_refs(c["x"], c["w"], c["b"], c["rm"], c["rv"], c["dy"], c["addend"])
    c.update(ref=ref, plain=plain, mask=mask, y_in=ref["y1"].float().contiguous(), mean_in=ref["mean"].float(), invstd_in=ref["invstd"].float())
    return c


# 16-bit storage on either side (the mixed-precision step): (x dtype, y dtype), None = fp32
H16_PAIRS = [("bf16", "bf16"), (None, "bf16"), ("bf16", None), ("f16", "f16"), (None, "f16")]
H16_SHAPES = [(777, 48), (1603, 256)]
TORCH_DT = {None: torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@functools.lru_cache(maxsize=None)
def train_h16_case(M, C, xdt, ydt):
    """The ordinary case with x / addend stored as xdt and dy / y as ydt: the float64 restatement of the STORED values (statistics and arithmetic of the kernel
    are fp32 on them; only the written y / dx are rounded).  The backward's mask is the stored y's sign."""
    c = dict(train_input(M, C, "ordinary"))
    tx, ty = TORCH_DT[xdt], TORCH_DT[ydt]
    c["x"], c["addend"], c["dy"] = c["x"].to(tx), c["addend"].to(tx), c["dy"].to(ty)
    ref0 = _train_restate(lambda v: v.double(), c["x"], c["w"], c["b"], c["rm"], c["rv"], c["dy"], None)
    y_in = ref0["y1"].to(ty).contiguous()
    ref, plain, mask = _train_refs(c["x"], c["w"], c["b"], c["rm"], c["rv"], c["dy"], c["addend"], y_in.float() > 0)
    c.update(ref=ref, plain=plain, mask=mask, y_in=y_in, mean_in=ref["mean"].float(), invstd_in=ref["invstd"].float(), xdt=xdt, ydt=ydt)
    return c


# ----------------------------------------------------------------------------------------------------------------------------------------
# re-drawing inside a decision margin
# ----------------------------------------------------------------------------------------------------------------------------------------
def _settle(g, draw, inside, what):
    """draw(mask) re-draws the inputs where mask is set; inside() -> the mask of entries inside a margin, from a fresh float64 forward."""
    for _ in range(50):
        bad = inside()
        if not bool(bad.any()):
            return
        draw(bad)
    raise AssertionError(what + ": entries stay inside the decision margin")


def _near_zero(pre):
    return pre.abs() < MARGIN * pre.abs().max()


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. kpf_bn2_add_relu_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
BN2_SHAPES = [(1, 8), (37, 8), (777, 48), (1603, 256), (515, 576), (300, 260)]


def _bn2_restate(t, c, mask):
    xa, xb, wa, ba, wb, bb = _leaves(t, c["xa"], c["xb"], c["wa"], c["ba"], c["wb"], c["bb"])
    rs = [t(v).clone() for v in (c["rma"], c["rva"], c["rmb"], c["rvb"])]
    pre = _bn(xa, wa, ba, rs[0], rs[1]) + _bn(xb, wb, bb, rs[2], rs[3])
    out = torch.relu(pre)
    ((pre * t(mask) if mask is not None else out) * t(c["dy"])).sum().backward()
    sa, sb = _stats(t(c["xa"])), _stats(t(c["xb"]))
    return {"out": out.detach(), "pre": pre.detach(), "stats": torch.stack((sa[0], sa[1], sb[0], sb[1])), "rma": rs[0], "rva": rs[1], "rmb": rs[2], "rvb": rs[3],
            "dxa": xa.grad, "dxb": xb.grad, "dwa": wa.grad, "dba": ba.grad, "dwb": wb.grad, "dbb": bb.grad}


@functools.lru_cache(maxsize=None)
def bn2_case(M, C):
    """out = relu(BN_a(xa) + BN_b(xb)): branch a wide and off-centre, branch b narrow; wb negative in every third channel.  No pre-activation within MARGIN of 0."""
    g = _gen(M, C, 41)
    xa, sa, ma = _rows(g, M, C)
    xb, sb, mb = _rows(g, M, C)
    wa, ba, rma, rva = _params(g, C)
    wb, bb, rmb, rvb = _params(g, C)
    wb = torch.where(torch.arange(C) % 3 == 0, -wb, wb)
    c = dict(xa=xa, xb=xb, wa=wa, ba=ba, wb=wb, bb=bb, rma=rma, rva=rva, rmb=rmb, rvb=rvb, dy=_dy(g, M, C), planted=None)
    pre64 = lambda: _bn(xa.double(), wa.double(), ba.double(), None, None) + _bn(xb.double(), wb.double(), bb.double(), None, None)

    def draw(bad):
        xa[bad] = (torch.randn(M, C, generator=g) * sa + ma)[bad]
        xb[bad] = (torch.randn(M, C, generator=g) * sb + mb)[bad]

    _settle(g, draw, lambda: _near_zero(pre64()), "bn2 %d x %d" % (M, C))
    ref = _bn2_restate(lambda v: v.double(), c, None)
    mask = ref["out"].float() > 0
    plain = _bn2_restate(lambda v: v.float(), c, mask)
    c.update(ref=ref, plain=plain, mask=mask, out_in=ref["out"].float().contiguous(), stats_in=ref["stats"].float().contiguous())
    return c


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. kpf_bn_relu_gmax_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
# (G, group, C, dmax_ld): group in {1, 7, 64, 256}; G below and above the 64 chunks of the backward's sums; dmax a column slice of a wider matrix
GMAX_SHAPES = [(5, 7, 8, 12), (33, 64, 48, 48), (70, 1, 48, 52), (3, 256, 12, 16), (130, 7, 260, 264)]


def first_argmax(z):
    """z [G][group][C] -> the first member that reaches the maximum."""
    group = z.shape[1]
    return torch.where(z == z.amax(1, keepdim=True), torch.arange(group).view(1, group, 1), group).amin(1)


def gmax_margins(pre, G, group):
    """From the float64 pre-activations [M][C]: per (group, channel) the distance that decides the winner — the maximum's lead over the largest DIFFERENT relu'd
    value (exact ties are duplicates: the first wins whatever the precision), or, where every member is <= 0, the distance of the largest member from 0."""
    p = pre.view(G, group, -1)
    z = torch.relu(p)
    top = z.amax(1)
    below = torch.where(z < top.unsqueeze(1), z, torch.full((), -float("inf"), dtype=z.dtype)).amax(1)
    return torch.where(top > 0, top - below, -p.amax(1))


@functools.lru_cache(maxsize=None)
def gmax_case(G, group, C, ld):
    """y[g][c] = max over the group's rows of relu(BN(x)), arg = the first winner.  Planted (group > 1): in group 0 rows m1 < m2 are equal and hold the maximum of
    every channel (arg = m1); the rows of group 1 lie on the side of the batch mean where w (x - mean) < 0, and every b is below -0.2: all its members are below
    zero in every channel (arg 0, value 0); w is negative in every fifth channel (the winner has the SMALLEST x)."""
    g = _gen(G, group, C, ld, 43)
    M = G * group
    x, sig, mu = _rows(g, M, C)
    w, b, rm, rv = _params(g, C)
    neg = torch.arange(C) % 5 == 0
    w = torch.where(neg, -w, w)
    b = -0.2 - b.abs()
    toward = torch.where(neg, -1.0, 1.0)  # the direction of x in which the pre-activation grows
    m1, m2 = (group // 3, group - 1) if group > 1 else (0, 0)
    fixed = torch.zeros(M, dtype=torch.bool)
    if group > 1:
        x[m1] = x[m2] = mu + 8.0 * sig * toward
        fixed[[m1, m2]] = True
        x[group:2 * group] = mu - (3.0 + torch.rand(group, C, generator=g)) * sig * toward
        fixed[group:2 * group] = True

    def inside():
        pre = _bn(x.double(), w.double(), b.double(), None, None)
        return (gmax_margins(pre, G, group) < MARGIN * pre.abs().max()).unsqueeze(1).expand(G, group, C).reshape(M, C)

    def draw(bad):
        bad = bad & ~fixed.unsqueeze(1)
        x[bad] = (torch.randn(M, C, generator=g) * sig + mu)[bad]

    _settle(g, draw, inside, "gmax %s" % ((G, group, C),))
    dmax = torch.randn(G, ld, generator=g)
    dmax[:, :C] = _dy(g, G, C)

    def run(t, arg, mask):
        xl, wl, bl = _leaves(t, x, w, b)
        r1, r2 = t(rm).clone(), t(rv).clone()
        pre = _bn(xl, wl, bl, r1, r2)
        z = torch.relu(pre).view(G, group, C)
        y = z.amax(1)
        if arg is None:
            arg = first_argmax(z.detach())
            mask = y.detach().float() > 0
        won = torch.gather(pre.view(G, group, C), 1, arg.unsqueeze(1)).squeeze(1)
        (won * t(mask) * t(dmax[:, :C])).sum().backward()
        m, s = _stats(t(x))
        return {"y": y.detach(), "pre": pre.detach(), "stats": torch.stack((m, s)), "rmean": r1, "rvar": r2, "dx": xl.grad, "dw": wl.grad, "db": bl.grad}, arg, mask

    ref, arg, mask = run(lambda v: v.double(), None, None)
    plain, _, _ = run(lambda v: v.float(), arg, mask)
    return dict(x=x, w=w, b=b, rm=rm, rv=rv, dmax=dmax, ref=ref, plain=plain, arg=arg.to(torch.uint8), mask=mask, m1=m1, m2=m2, neg=neg, planted=None,
                y_in=ref["y"].float().contiguous(), stats_in=ref["stats"].float().contiguous(), tie_group=0 if group > 1 else None,
                dead_group=1 if group > 1 else None)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. kpf_bn_ssr_forward / _backward
# ----------------------------------------------------------------------------------------------------------------------------------------
# (rows, C, n1, n2): the classes of the training step (three siblings and a second sum; two; one and two; four), C = 256 (64 quads: one row lane), n = 4 with n2 > 0
SSR_SHAPES = [(4096, 128, 3, 1), (672, 128, 2, 0), (77, 24, 1, 2), (33, 8, 4, 0), (131, 256, 1, 1), (97, 16, 2, 2)]


def _ssr_sums(y, rows, C, n1, n2):
    yv = y.view(rows, n1 + n2, C)
    return yv[:, :n1].sum(1), (yv[:, n1:].sum(1) if n2 else None)


def _ssr_restate(t, c, masks):
    rows, C, n1, n2 = c["shape"]
    xl, wl, bl = _leaves(t, c["x"], c["w"], c["b"])
    r1, r2 = t(c["rm"]).clone(), t(c["rv"]).clone()
    s1, s2 = _ssr_sums(_bn(xl, wl, bl, r1, r2), rows, C, n1, n2)
    out = torch.relu(s1) if not n2 else torch.relu(torch.relu(s1) + s2)
    if masks is None:
        fixed = out
    else:  # d = dout (out > 0) reaches S2; d (S1 > 0) reaches S1
        m_out, m_s1 = (t(m) for m in masks)
        fixed = s1 * m_out if not n2 else (s1 * m_s1 + s2) * m_out
    (fixed * t(c["dout"])).sum().backward()
    m, s = _stats(t(c["x"]))
    return {"out": out.detach(), "s1": s1.detach(), "pre": (s1 if not n2 else torch.relu(s1) + s2).detach(), "stats": torch.stack((m, s)), "rmean": r1, "rvar": r2,
            "dx": xl.grad, "dw": wl.grad, "db": bl.grad}


@functools.lru_cache(maxsize=None)
def ssr_case(rows, C, n1, n2):
    """x [rows][n C]: n = n1 + n2 sibling blocks side by side; out = relu(S1) or relu(relu(S1) + S2).  No S1 and no final pre-activation within MARGIN of 0."""
    g = _gen(rows, C, n1, n2, 47)
    n = n1 + n2
    x, sig, mu = _rows(g, rows, n * C)
    w, b, rm, rv = _params(g, n * C)
    w = torch.where(torch.arange(n * C) % 7 == 3, -w, w)
    c = dict(x=x, w=w, b=b, rm=rm, rv=rv, dout=_dy(g, rows, C), shape=(rows, C, n1, n2), planted=None)

    def inside():
        s1, s2 = _ssr_sums(_bn(x.double(), w.double(), b.double(), None, None), rows, C, n1, n2)
        bad = _near_zero(s1)
        if n2:
            bad |= _near_zero(torch.relu(s1) + s2)
        return bad.repeat(1, n)

    def draw(bad):
        x[bad] = (torch.randn(rows, n * C, generator=g) * sig + mu)[bad]

    _settle(g, draw, inside, "ssr %s" % ((rows, C, n1, n2),))
    ref = _ssr_restate(lambda v: v.double(), c, None)
    masks = (ref["out"].float() > 0, ref["s1"] > 0)
    plain = _ssr_restate(lambda v: v.float(), c, masks)
    c.update(ref=ref, plain=plain, masks=masks, out_in=ref["out"].float().contiguous(), stats_in=ref["stats"].float().contiguous())
    return c
