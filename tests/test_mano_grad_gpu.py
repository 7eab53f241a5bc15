"""kpf_mano_backward_f32 and the training path built on it (heads_train.ManoLayerHip) against float64 autograd of the oracle's restatement
(tests/mano_cases.py).  The bound of every gradient comparison is the project's rule for fp32 kernels: e_kernel <= 4 e_plain + 8 * 2^-24, e_plain being the
distance of fp32 torch-CPU autograd of the same restatement from the float64 one.

Measured on the MI355X (e_kernel / e_plain, relative to max|ref64|): see DESIGN.md 4.11."""
import os

import numpy as np
import pytest
import torch

import mano_cases as M
from conftest import GOLDEN
from test_heads_gpu import _dev, _train_step_check, rel_err
from test_heads_oracle import mano_case

pytestmark = pytest.mark.gpu


def _model(dev):
    from keypointfusion_amd.heads import mano_model_arrays
    return mano_model_arrays(M.model_sd(), dev)


def _backward(dev, pose6d, betas, grads, ld6=96, ldb=10, ldd6=96, lddb=10):
    """-> (d_pose6d [B, 96], d_betas [B, 10]) of one kpf_mano_backward_f32 call; grads: four tensors or None"""
    from keypointfusion_amd import lib as L
    B = pose6d.shape[0]
    p6, bt = pose6d.to(dev).contiguous(), betas.to(dev).contiguous()
    gs = [None if g is None else g.to(dev).contiguous() for g in grads]
    d6, db = torch.full((B, 96), float("nan"), device=dev), torch.full((B, 10), float("nan"), device=dev)
    L.check(L.load().kpf_mano_backward_f32(p6.data_ptr(), ld6, bt.data_ptr(), ldb, *[m.data_ptr() for m in _model(dev)],
                                           *[None if g is None else g.data_ptr() for g in gs], d6.data_ptr(), ldd6, db.data_ptr(), lddb, B,
                                           torch.cuda.current_stream().cuda_stream), "kpf_mano_backward_f32")
    return d6, db


def _check(tag, errs):
    for name, (ek, ep) in errs.items():
        print("MANO-GRAD %-22s %-8s e_kernel %.3e e_plain %.3e%s" % (tag, name, ek, ep, "" if M.within(ek, ep) else " MISSES"))
    for name, (ek, ep) in errs.items():
        assert M.within(ek, ep), (tag, name, ek, ep)


def test_backward_matches_float64_autograd():
    dev = _dev()
    c = M.grad_case()
    assert all(bool(torch.isfinite(r).all()) for r in c.ref)
    d6, db = _backward(dev, c.pose6d, c.betas, c.projs)
    _check("all outputs", M.errors(c, d6, db))


@pytest.mark.parametrize("which", range(4))
def test_each_gradient_input_alone(which):
    dev = _dev()
    c = M.grad_case()
    ref, plain = c.single[which]
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    d6, db = _backward(dev, c.pose6d, c.betas, [p if i == which else None for i, p in enumerate(c.projs)])
    _check(M.OUTPUTS[which] + " alone", M.errors(c, d6, db, ref, plain))


def test_strided_rows_and_guards():
    """The eval plan's layout: rows of 108 floats, pose6d in columns 0..95 and betas from column 96; the gradient rows likewise.  Columns the kernel does not own
    and 64 guard floats behind each output keep their canary."""
    from keypointfusion_amd import lib as L
    dev = _dev()
    c = M.grad_case()
    B, CAN = 5, 777.25
    rows = torch.zeros(B, 108)
    rows[:, :96], rows[:, 96:106] = c.pose6d, c.betas
    rows = rows.to(dev)
    out = torch.full((B * 108 + 64,), CAN, device=dev)
    gs = [p.to(dev).contiguous() for p in c.projs]
    L.check(L.load().kpf_mano_backward_f32(rows.data_ptr(), 108, rows.data_ptr() + 96 * 4, 108, *[m.data_ptr() for m in _model(dev)], *[g.data_ptr() for g in gs],
                                           out.data_ptr(), 108, out.data_ptr() + 96 * 4, 108, B, torch.cuda.current_stream().cuda_stream), "kpf_mano_backward_f32")
    o = out[:B * 108].view(B, 108)
    assert bool((o[:, 106:] == CAN).all()) and bool((out[B * 108:] == CAN).all())
    d6, db = _backward(dev, c.pose6d, c.betas, c.projs)
    assert torch.equal(o[:, :96], d6) and torch.equal(o[:, 96:106], db)
    # dense outputs with guards of their own
    g6, gb = torch.full((B * 96 + 64,), CAN, device=dev), torch.full((B * 10 + 64,), CAN, device=dev)
    p6, bt = c.pose6d.to(dev), c.betas.to(dev)
    L.check(L.load().kpf_mano_backward_f32(p6.data_ptr(), 96, bt.data_ptr(), 10, *[m.data_ptr() for m in _model(dev)], *[g.data_ptr() for g in gs],
                                           g6.data_ptr(), 96, gb.data_ptr(), 10, B, torch.cuda.current_stream().cuda_stream), "kpf_mano_backward_f32")
    assert bool((g6[B * 96:] == CAN).all()) and bool((gb[B * 10:] == CAN).all())
    assert torch.equal(g6[:B * 96].view(B, 96), d6) and torch.equal(gb[:B * 10].view(B, 10), db)


def test_identity_rotation_gets_the_finite_limit():
    dev = _dev()
    c = M.identity_case()
    assert all(bool(torch.isfinite(r).all()) for r in c.ref)
    d6, db = _backward(dev, c.pose6d, c.betas, c.projs)
    assert bool(torch.isfinite(d6).all()) and bool(torch.isfinite(db).all())
    _check("identity", M.errors(c, d6, db))


def test_backward_is_deterministic_and_independent_of_the_batch():
    dev = _dev()
    c = M.grad_case()
    a = _backward(dev, c.pose6d, c.betas, c.projs)
    b = _backward(dev, c.pose6d, c.betas, c.projs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for i in range(5):
        s = _backward(dev, c.pose6d[i:i + 1], c.betas[i:i + 1], [p[i:i + 1] for p in c.projs])
        assert torch.equal(s[0][0], a[0][i]) and torch.equal(s[1][0], a[1][i]), i


def test_mano_layer_hip_forward_is_the_forward_kernel():
    from keypointfusion_amd import lib as L
    from keypointfusion_amd.heads_train import ManoLayerHip
    dev = _dev()
    c = M.grad_case()
    B = 5
    p6, bt, model = c.pose6d.to(dev), c.betas.to(dev), _model(dev)
    outs = ManoLayerHip.apply(p6.clone().requires_grad_(True), bt.clone().requires_grad_(True), *model)
    direct = [torch.empty(B, 778, 3, device=dev), torch.empty(B, 21, 3, device=dev), torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 48, device=dev)]
    L.check(L.load().kpf_mano_forward_f32(p6.data_ptr(), 96, bt.data_ptr(), 10, *[m.data_ptr() for m in model], *[d.data_ptr() for d in direct], B,
                                          torch.cuda.current_stream().cuda_stream), "kpf_mano_forward_f32")
    for o, d in zip(outs, direct):
        assert o.shape == d.shape and torch.equal(o.detach(), d)
    assert all(o.requires_grad for o in outs)


def _head(dev):
    from keypointfusion_amd.model.mano_head import mano_regHead
    m = mano_regHead()
    m.load_state_dict(mano_case()[0], strict=True)
    return m.to(dev).train()


def test_hip_layer_train_step_matches_the_reference_step():
    """The checks of test_heads_gpu.test_mano_head_train_mode_matches_the_reference_step, on layer="hip", through the drop-in module's attribute."""
    from keypointfusion_amd.weights import synthetic_tensor
    dev = _dev()
    g = np.load(os.path.join(GOLDEN, "aux_train.npz"))
    m = _head(dev)
    assert m.hip_mano_layer is False
    m.hip_mano_layer = True
    feats = torch.from_numpy(synthetic_tensor((4, 1024), 5, "mano_features_train")).to(dev).requires_grad_(True)
    r = m(feats)
    keys = ("verts3d", "joints3d", "mano_shape", "mano_pose", "mano_pose_aa")
    for k in keys:
        assert rel_err(r[k], g["mano_" + k]) < 1e-4, k
    _train_step_check(m, [r[k] for k in keys], feats, "mano", g, 1e-3)


def test_hip_and_torch_layers_give_the_same_feature_gradient():
    """layer="torch" against "hip" on one batch: the `features` gradient element-wise, float64 autograd of the whole head (oracle.aux_oracle.mano_head_forward) as
    the reference and fp32 torch-CPU autograd of it as e_plain."""
    from keypointfusion_amd.heads_train import mano_head_train_forward
    from keypointfusion_amd.weights import synthetic_tensor
    from oracle import aux_oracle as A
    dev = _dev()
    m = _head(dev)
    sd = mano_case()[0]
    feats = torch.from_numpy(synthetic_tensor((4, 1024), 5, "mano_features_train"))
    keys = ("verts3d", "joints3d", "mano_pose", "mano_pose_aa", "mano_shape")
    gen = torch.Generator().manual_seed(31)
    projs = {k: torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1 for k, s in zip(keys, ((4, 778, 3), (4, 21, 3), (4, 16, 3, 3), (4, 48), (4, 10)))}

    def cpu_grad(dtype):
        x = feats.to(dtype).requires_grad_(True)
        out = A.mano_head_forward(M._cast(sd, dtype), x)
        return torch.autograd.grad(sum((out[k] * projs[k].to(dtype)).sum() for k in keys), x)[0]

    ref, plain = cpu_grad(torch.float64), cpu_grad(torch.float32)
    assert bool(torch.isfinite(ref).all())
    den = float(ref.abs().max())
    e_plain = float((plain.double() - ref).abs().max()) / den
    got = {}
    for layer in ("torch", "hip"):
        x = feats.to(dev).requires_grad_(True)
        out = mano_head_train_forward(m, x, layer=layer)
        got[layer] = torch.autograd.grad(sum((out[k].double() * projs[k].to(dev)).sum() for k in keys), x)[0].cpu().double()
        ek = float((got[layer] - ref).abs().max()) / den
        print("MANO-GRAD head features layer=%-5s e_kernel %.3e e_plain %.3e" % (layer, ek, e_plain))
    for layer in ("torch", "hip"):
        assert M.within(float((got[layer] - ref).abs().max()) / den, e_plain), layer
    with pytest.raises(ValueError):
        mano_head_train_forward(m, feats.to(dev), layer="triton")
