"""Runs every case builder of tests/train_head_cases.py on the CPU and asserts, from the float64 reference alone, that each case is in the regime it is named
for: what tests/test_train_head_kernels_gpu.py then compares can see the faults it is there to see.  No GPU."""
import pytest
import torch

import train_head_cases as TC
from oracle import kpf_oracle as O


def _finite(case):
    for side in ("ref", "plain"):
        for k, v in case[side].items():
            assert bool(torch.isfinite(v).all()), (side, k)
            assert v.dtype == (torch.float64 if side == "ref" else torch.float32), (side, k)
    for k in case["ref"]:
        assert float(case["ref"][k].abs().max()) > 0, k
        assert TC.rel_err(case["plain"][k], case["ref"][k]) < 1e-3, k  # the operation is well conditioned here: the comparison means something


@pytest.mark.parametrize("std,sigma", TC.HEATMAP_STD_SIGMA)
@pytest.mark.parametrize("B,J,Fs", TC.HEATMAP_SHAPES)
def test_heatmap_case(B, J, Fs, std, sigma):
    c = TC.heatmap_case(B, J, Fs, std, sigma)
    _finite(c)
    hm64, hm32 = c["ref"]["hm"], c["plain"]["hm"]
    assert bool(torch.equal(hm32, O.joint2heatmap(c["uvd"][:, :, :2], std, Fs, sigma=sigma)))  # the two oracles state the same map
    assert float(hm64[:, c["centre"]].amax((-1, -2)).min()) > 1 - 1e-9      # the joint on a pixel centre (to the rounding of its fp32 coordinate)
    assert 0.1 < float(hm64[:, c["border"]].amax((-1, -2)).min()) < 1.0     # the border joint lights the corner pixel
    assert float(hm64[:, c["off"]].max()) < 0.5
    if c["underflows"]:  # every fp32 value of the far joint's map is 0: the exact values lie below the smallest fp32 subnormal
        assert float(hm32[:, c["far"]].abs().max()) == 0.0 and float(hm64[:, c["far"]].max()) < 2.0 ** -150
        assert float(c["plain"]["duvd"][:, c["far"]].abs().max()) == 0.0
    assert float(c["ref"]["duvd"][..., 2].abs().max()) == 0.0
    assert bool((c["uvd"][:, :, :2].abs() > 1).any()) and bool((c["uvd"][:, :, :2].abs() < 1).any())


@pytest.mark.parametrize("B,J,P", TC.GATE_SHAPES)
def test_geom_gate_case(B, J, P):
    c = TC.geom_gate_case(B, J, P)
    _finite(c)
    gam = c["ref"]["gam"]
    if c["planted"]:
        assert float(gam[:, 0, 0].min()) == 1.0
        assert 0.5e-4 < float(gam[:, J - 1, P - 1].max()) < 2e-4


@pytest.mark.parametrize("half_size", [64.0, 128.0])
@pytest.mark.parametrize("flip", [1.0, -1.0])
@pytest.mark.parametrize("B,J,P", TC.GATE_SHAPES)
def test_geom_gate_uvd_case(B, J, P, flip, half_size):
    c = TC.geom_gate_uvd_case(B, J, P, flip, half_size)
    _finite(c)
    cam, cube, center, Minv = c["cam"], c["cube"], c["center"], c["Minv"]
    assert bool(((cam[:, 0] - cam[:, 1]).abs() > 20).all()) and bool(((cam[:, 2] - cam[:, 3]).abs() > 20).all())
    assert bool((cube == torch.tensor([250.0, 200.0, 300.0])).all())
    assert bool((center[:, :2].abs() > 10).all())
    assert bool((Minv[:, :2, 2].norm(dim=1) > 100).all()), "translation"
    assert bool((Minv[:, 0, 1].abs() > 0.05 * Minv[:, 0, 0].abs()).all()) and bool(((Minv[:, 0, 1] + Minv[:, 1, 0]).abs() > 0.02 * Minv[:, 0, 0].abs()).all()), "rotation and shear"
    assert float((c["M"] @ Minv.double() - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-9
    assert float(c["ref"]["xyz"].abs().max()) < 3.0  # the joints land in and around the cube
    if c["planted"]:
        assert float(c["ref"]["gam"][:, 0, 0].min()) > 1 - 1e-5
        assert 0.5e-4 < float(c["ref"]["gam"][:, J - 1, P - 1].max()) < 2e-4
    # a kernel that confused fx with fy, cube_x with cube_y, or the sign of flip computes something this case tells apart from the reference
    d64 = lambda t: t.double()
    others = {"fx<->fy": TC._uvd_restate(c, d64, flip, "f"), "cube_x<->cube_y": TC._uvd_restate(c, d64, flip, "cube"), "flip": TC._uvd_restate(c, d64, -flip)}
    for name in ("gam", "duvd"):
        for what, o in others.items():
            moved = TC.rel_err(o[name], c["ref"][name])
            assert moved > 100 * TC.bound(c, name), (what, name, moved, TC.bound(c, name))


@pytest.mark.parametrize("kernel", [0.8, 0.6])
@pytest.mark.parametrize("B,N,J", sorted({s[:3] for s in TC.POSE_SHAPES}))
def test_pose_case(B, N, J, kernel):
    c = TC.pose_case(B, N, J, kernel)
    _finite(c)
    cmp_, m32, m64, clos, dis, off = c["compared"], c["mask32"], c["mask64"], c["clos_unmasked"], c["dis"], c["ref"]["off"]
    assert c["left_out"] <= 0.01, c["left_out"]
    assert bool((m64 == m32)[cmp_].all())  # away from the radius the decision does not depend on the precision
    for b, n, j in c["inside"] + c["outside"] + c["on_joint"]:
        assert bool(cmp_[b, n, j]), (b, n, j)
    for b, n in c["z_masked"] + c["z_kept"]:
        assert bool(cmp_[b, n].all())
    assert all(bool(m64[b, n, j]) for b, n, j in c["inside"]) and not any(bool(m64[b, n, j]) for b, n, j in c["outside"])
    assert all(abs(float(clos[b, n, j])) < 2e-3 for b, n, j in c["inside"] + c["outside"])
    assert any(abs(float(clos[b, n, j])) < 1e-4 for b, n, j in c["inside"]) and any(abs(float(clos[b, n, j])) < 1e-4 for b, n, j in c["outside"])
    for b, n, j in c["on_joint"]:
        assert float(dis[b, j, n]) == 0.0 and float(off[b, n, 3 * J + j]) == 1.0 and not bool(off[b, n, 3 * j:3 * j + 3].any())
    zj = c["z_joint"]
    assert not any(bool(m64[b, n].any()) for b, n in c["z_masked"]) and all(bool(m64[b, n, zj]) for b, n in c["z_kept"])
    assert all(float(clos[b, n, zj]) > 0.3 for b, n in c["z_masked"])  # only their z masks them
    assert len(c["z_masked"]) >= B and (N < 16 or len(c["z_kept"]) >= B)
    assert 0.02 < float(m64.double().mean()) < 0.98  # both decisions occur


@pytest.mark.parametrize("B,J,P,wdis,with_dsw", TC.GATE_MIX_CASES)
def test_gate_mix_case(B, J, P, wdis, with_dsw):
    c = TC.gate_mix_case(B, J, P, wdis, with_dsw)
    _finite(c)
    sat = c["saturated"]
    assert 0.03 < float(sat.double().mean()) < 0.2
    lg = c["logits"]
    assert bool((lg[sat].abs() == 30).all()) and bool((lg[sat] > 0).any()) and bool((lg[sat] < 0).any())
    sw32 = c["plain"]["sw"].permute(0, 2, 1).reshape(B * P, J)
    assert bool((sw32[sat & (lg > 0)] == 1.0).all()) and float(sw32[sat & (lg < 0)].max()) < 1e-12  # the fp32 sigmoid is saturated
    dl = c["ref"]["d_logits"]
    assert float(dl[sat].abs().max()) < 1e-10 * float(dl.abs().max())
    assert (c["d_sw"] is not None) == with_dsw


def test_gate_mix_cases_reach_every_path():
    shapes = {(B, J, P) for B, J, P, _, _ in TC.GATE_MIX_CASES}
    assert any(P < 8 and B * J < 32 for B, J, P in shapes) and any(P % 256 and P % 8 and P > 256 for B, J, P in shapes)
    assert {w for _, _, _, w, _ in TC.GATE_MIX_CASES} == {-3.0, 0.3, 6.0} and {d for *_, d in TC.GATE_MIX_CASES} == {True, False}
    assert len({J for _, J, _ in shapes}) > 1


@pytest.mark.parametrize("rows,group,C,dy_ld", TC.GROUP_MAX_SHAPES)
def test_group_max_case(rows, group, C, dy_ld):
    c = TC.group_max_case(rows, group, C)
    x, y, arg = c["x"], c["y"], c["arg"].long()
    assert bool(torch.equal(torch.gather(x, 1, arg.unsqueeze(1)).squeeze(1), y))
    before = torch.arange(group).view(1, group, 1) < arg.unsqueeze(1)
    assert bool((x[before.expand_as(x)] < y.unsqueeze(1).expand_as(x)[before.expand_as(x)]).all())  # nothing in front of arg reaches the maximum
    assert bool((arg[1] == 0).all()) and bool((x[1] == x[1, 0, 0]).all())
    if group > 1:
        assert c["m1"] < c["m2"] and bool((arg[0] == c["m1"]).all()) and bool(torch.equal(x[0, c["m1"]], x[0, c["m2"]]))
        assert float(((x == y.unsqueeze(1)).sum(1) > 1).double().mean()) > 0.3  # many repeated maxima
    assert bool(torch.equal(c["dx"].sum(1), c["dy"])) and int((c["dx"] != 0).sum()) <= rows * C and dy_ld >= C


@pytest.mark.parametrize("N", TC.BALL_NS)
def test_ball_group_case(N):
    c = TC.ball_group_case(N)
    _finite(c)
    assert c["margin"] > TC.BALL_MARGIN, c["margin"]
    assert bool(torch.equal(c["idx"], c["idx64"]))  # so the index sets do not depend on the precision
    mem, idx, J = c["members"], c["idx"], TC.BALL_J
    assert bool((mem[:, :, 0] == 1).all()) and bool((idx[:, :, 0] == N).all())  # a ball with its own centre alone
    assert c["crowded"] == (N == 130)
    if c["crowded"]:  # truncated to the first 64 in index order: more members than slots, the slots ascending
        assert bool((mem[2, :, 1] > 64).all())
        assert bool((idx[2, :, 1, 1:] > idx[2, :, 1, :-1]).all())
    assert bool((mem >= 1).all()) and bool((mem[:, :, 1:] < 64).any())  # unfilled slots repeat the first member somewhere
    for b, ri, n, inside in c["pairs"]:
        f = float(c["d2"][b, 2, n] / c["r2"][ri]) ** 0.5
        assert abs(f - (1 - 1e-3 if inside else 1 + 1e-3)) < 1e-5, (b, ri, n, f)
        assert bool((idx[ri, b, 2] == n).any()) == inside
    assert float(c["ref"]["GX"][:, 3::4].abs().max()) == 0.0


def test_ball_bwd_case_list_lengths():
    idx, counts = TC.ball_bwd_indices()
    B, N, Jn = (TC.BALL_BWD[k] for k in ("B", "N", "Jn"))
    assert idx.shape == (3, B, Jn * 64) and int(idx.min()) >= 0 and int(idx.max()) < N + Jn
    have = set(counts.flatten().tolist())
    assert set(TC.BALL_BWD_COUNTS) <= have, sorted(set(TC.BALL_BWD_COUNTS) - have)
    assert int(counts[:, :, :N].max()) >= 129 and int(counts[:, :, N:].max()) >= 129  # a point row and a joint row among the heavy ones
    for ld3 in TC.BALL_BWD_LD3:
        c = TC.ball_bwd_case(ld3)
        _finite(c)
        start, lst = TC.stable_inverse(idx.view(3 * B, -1), N + Jn)
        assert bool(torch.equal((start[:, 1:] - start[:, :-1]).view(3, B, -1), counts.int()))


@pytest.mark.parametrize("B,P,R,G,C,with_w", TC.GATHER_CASES)
def test_gather_case(B, P, R, G, C, with_w):
    c = TC.gather_case(B, P, R, G, C, with_w)
    _finite(c)
    idx, start, lst, cnt = c["idx"], c["start"], c["list"], c["counts"]
    assert int(idx.min()) >= 0 and int(idx.max()) == P - 1 and bool((cnt == 0).any())
    assert bool((start[:, 0] == 0).all()) and bool((start[:, -1] == R * G).all())
    for b in range(B):
        keys = idx[b][lst[b].long()]
        assert bool((keys[1:] >= keys[:-1]).all())
        assert bool(((lst[b][1:] > lst[b][:-1]) | (keys[1:] > keys[:-1])).all())  # ascending entries within a row
    E = R * G
    if P > 2048:  # every one of the 8 waves of the inversion owns entries
        seg = ((E + 7) // 8 + 63) // 64 * 64
        assert 7 * seg < E
    if P == 3:
        assert int(cnt.max()) == E == 8192
    assert (c["w"] is not None) == with_w


def test_gather_cases_reach_every_path():
    cs = TC.GATHER_CASES
    assert any(P > 2048 for _, P, *_ in cs) and any(C // 4 > 32 and (C // 4) % 64 for *_, C, _ in cs) and any(C // 4 > 64 for *_, C, _ in cs) and any(C // 4 < 32 for *_, C, _ in cs)
    assert {w for *_, w in cs} == {True, False}
    for w in (True, False):
        _finite(TC.gather_cols_case(w))


@pytest.mark.parametrize("kind", ["soft", "sharp"])
@pytest.mark.parametrize("scale", TC.ATTN_SCALES)
@pytest.mark.parametrize("B,H", sorted({s[:2] for s in TC.ATTN_SHAPES}))
def test_attn_case(B, H, scale, kind):
    c = TC.attn_case(B, H, scale, kind)
    _finite(c)
    P = c["ref"]["P"]
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    if kind == "sharp":
        assert c["sharp_share"] > 0.5, c["sharp_share"]
        q, k = c["q"].double().view(B, 21, H, 32).transpose(1, 2), c["k"].double().view(B, 21, H, 32).transpose(1, 2)
        assert 10 < float((scale * q @ k.transpose(-1, -2)).std()) < 20
    else:
        assert c["sharp_share"] < 0.5  # (scale = 1 on N(0, 1) operands already has logits of standard deviation 5.7)
    keep = (torch.rand(B, H, 21, 21, generator=torch.Generator().manual_seed(1)) >= 0.25).to(torch.uint8)
    r64, r32 = TC.attn_dropout_refs(B, H, scale, kind, keep, 0.25)
    assert bool(torch.equal(r64["P"], P)) and not bool(torch.equal(r64["ctx"], c["ref"]["ctx"]))
    assert all(bool(torch.isfinite(v).all()) for v in list(r64.values()) + list(r32.values()))
