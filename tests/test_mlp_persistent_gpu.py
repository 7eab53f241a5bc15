"""The persistent fp32 ConvNeXt MLP kernel (the default behind kpf_convnext_mlp_f32 at C = 96 / 128) against the one-tile-per-workgroup
kernel it replaces (KPF_MLP_V1=1): same bits, for every row count and with `out` aliasing `x` or not; against an fp64 restatement of the
block's MLP at the bound tests/test_parity_gpu.py::test_fused_convnext_mlp uses; and independence of a row's bits from M and from the
row's position (tile, wave, lane) in the launch.

Both kernels feed every accumulator the same MFMA sequence (GEMM1: 16-deep steps ascending; GEMM2: hidden tiles ascending), so equality
is exact, not a tolerance."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MS = [1, 100, 128, 129, 4133, 262144]


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from keypointfusion_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _operands(C, M, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, C, generator=g)
    x = torch.randn(M, C, generator=g)
    w1 = torch.randn(4 * C, C, generator=g) / C ** 0.5
    b1 = torch.randn(4 * C, generator=g) * 0.5
    w2 = torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5
    b2 = torch.randn(C, generator=g)
    gam = torch.rand(C, generator=g)
    return y, x, w1, b1, w2, b2, gam


def _run(d, out, M, C):
    """d = (y, x, w1, b1, w2, b2, gamma) on the device; rows [0, M) of y / x / out."""
    from keypointfusion_amd import engine as E, lib as L
    L.check(L.load().kpf_convnext_mlp_f32(*[E._ptr(t) for t in d], E._ptr(out), M, C, E._stream()), "kpf_convnext_mlp_f32")
    torch.cuda.synchronize()


@pytest.mark.parametrize("alias", [False, True], ids=["out_separate", "out_is_x"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("C", [96, 128])
def test_persistent_equals_v1_bit_for_bit(C, M, alias, monkeypatch):
    dev = _dev()
    host = _operands(C, M, 1000 * C + M % 997)
    outs = []
    for v1 in ("1", "0"):
        monkeypatch.setenv("KPF_MLP_V1", v1)
        d = [t.to(dev) for t in host]  # fresh x per run: the aliased call overwrites it
        out = d[1] if alias else torch.full((M + 1, C), 7.0, device=dev)  # one guard row behind the last
        _run(d, out, M, C)
        if not alias:
            assert bool((out[M] == 7.0).all()), "wrote past row M"
            assert torch.equal(d[1], host[1].to(dev)), "x changed although out does not alias it"
        outs.append(out[:M].clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("C,M", [(96, 129), (96, 4133), (128, 100), (128, 4133)])
def test_persistent_matches_fp64(C, M, monkeypatch):
    monkeypatch.delenv("KPF_MLP_V1", raising=False)
    dev = _dev()
    y, x, w1, b1, w2, b2, gam = host = _operands(C, M, C + M)
    ref = x.double() + gam.double() * (F.gelu(y.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double())
    d = [t.to(dev) for t in host]
    _run(d, d[1], M, C)  # in place, as the engine calls it
    e = float((d[1].cpu().double() - ref).abs().max() / ref.abs().max())
    print("C=%d M=%d rel err vs fp64 %.3e" % (C, M, e))
    assert e < 1e-5, e


@pytest.mark.parametrize("C", [96, 128])
def test_row_bits_do_not_depend_on_m_or_position(C, monkeypatch):
    """The same rows inside launches of different M, and at another tile / wave / lane position, give the same bits."""
    monkeypatch.delenv("KPF_MLP_V1", raising=False)
    dev = _dev()
    M = 40000  # more tiles than the persistent grid has workgroups: rows are also reached in a workgroup's second pass
    host = _operands(C, M, 7 * C)
    d = [t.to(dev) for t in host]
    full = torch.empty(M, C, device=dev)
    _run(d, full, M, C)
    for first, n in ((0, 300), (0, 4133), (37, 500), (128 * 300 + 5, 1595)):
        sub = [d[0][first:first + n], d[1][first:first + n]] + d[2:]
        out = torch.empty(n, C, device=dev)
        _run(sub, out, n, C)
        assert torch.equal(out.view(torch.int32), full[first:first + n].view(torch.int32)), (first, n)
