"""Every form of the weight-gradient GEMM (csrc/kpf_wgrad.hip: kpf_conv2d_wgrad) forced through kpf_conv2d_wgrad_force_form on small ragged shapes and pinned to
torch's float64 conv2d backward on the CPU — the backward twin of test_igemm_tiles_gpu.py.  The cases of test_kernels_train_gpu.py run the (2, 2) fp32 tile (one
case the (4, 2) tile) and the 64-tile 16-bit kernel; the tiles the training step of the benchmark runs, the 128-tile 16-bit kernel and the forms behind
environment switches are pinned here.  Shapes, operands and references: wgrad_forms.py.

What is asserted:
 1. accuracy, for dw and for db: e_kernel <= 4 * e_plain + 8 * 2^-24 (test_fusion_head_kernels_gpu.py, test_igemm_tiles_gpu.py), both errors relative to
    max|ref64|, e_plain = the same backward in fp32 on the CPU.  16-bit storage: the reference takes the operands as stored; KPF_DT_F32_MMA_*: the products on the
    rounded operands (exact in fp32, so the same bound), the bias gradient on dy as given (the kernel sums what it loads, before rounding).
 2. canaries: a quiet NaN with a payload survives behind the last element of dw and of db (the trimmed shapes included) and behind the workspace at exactly the
    size kpf_conv2d_wgrad_plan names; outputs that start as NaN come back finite and the operands' pad columns are NaN: every output was written, no pad was read.
 3. bits: channel-stacked groups of fp32 operands equal the per-group calls on every tile (include/kpf.h); a descriptor + kpf_wgrad_reduce_multi equals the
    immediate reduce; an unforced call equals the forced call on the form the query names; KPF_DT_F32_MMA_* on a tile without the 16-bit kernel equals the fp32 call.
 4. the forms behind KPF_WG16_FORM, KPF_WG16_RING, KPF_WG16S_RING, KPF_WGRAD_H16_WIDEN, KPF_WG16S_XCD (read once per process): one fresh child each
    (wgrad_forms_child.py), held to 1 and 2.
test_forms_have_every_kind_of_workgroup (no GPU) proves through the plan query that every forced form has interior and ragged workgroups in N and in K, a split and
a ragged last stage on these shapes, that the few-pixels rule selects the 128-tile kernel, and prints the forms of the benchmark's training step.
One line per comparison ("WGRAD form variant type ..."); profiles/wgrad_form_errors.txt is one run on the MI355X."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import wgrad_forms as WF
from wgrad_forms import VARIANTS, variant

F32_FORMS = {"f32_2x2": (2, 2), "f32_2x4": (2, 4), "f32_4x2": (4, 2), "f32_4x4": (4, 4)}
H16_FORMS = ("h16s", "h16")
ENV_FORMS = {  # setting -> the family the query must name for 16-bit operands under it
    "KPF_WG16_FORM=128": "h16", "KPF_WG16_FORM=128 KPF_WG16_RING=4": "h16", "KPF_WG16S_RING=3": "h16s", "KPF_WGRAD_H16_WIDEN=1": "f32", "KPF_WG16S_XCD=0": "h16s"}

# The weight-gradient GEMMs of one training step of the benchmark (KPFusion-convnext-tiny, 128 x 128 crops, B = 32: bench.py's train128 / train128_bf16), recorded
# from the kpf_conv2d_wgrad calls one eager step makes.  Two channel-stacked groups: the paired backbones; the fusion head's layers stay fp32 in the bf16 step.
BENCH_SHAPES = [  # groups, M, N, K, 1x1, trimmed, calls per step, dtype in the fp32 step, dtype in the bf16 step (None: not in that step)
    (1, 43008, 128, 4, 1, 1, 6, 'F32', 'F32'),
    (3, 43008, 128, 128, 1, 0, 4, 'F32', 'F32_MMA_BF16'),
    (1, 32768, 24, 152, 1, 1, 2, 'F32', 'F32'),
    (1, 32768, 96, 64, 0, 0, 2, 'F32', None),
    (1, 32768, 96, 128, 0, 0, 2, None, 'BF16'),
    (1, 32768, 128, 4, 1, 1, 2, 'F32', 'F32'),
    (1, 32768, 128, 108, 1, 1, 2, 'F32', 'F32'),
    (1, 32768, 128, 128, 1, 0, 4, 'F32', 'F32'),
    (2, 32768, 48, 96, 1, 0, 1, 'F32', 'BF16'),
    (2, 32768, 48, 432, 0, 0, 1, 'F32', 'BF16'),
    (2, 32768, 64, 128, 1, 0, 1, 'F32', 'BF16'),
    (2, 32768, 64, 288, 1, 0, 1, 'F32', 'BF16'),
    (2, 32768, 64, 576, 0, 0, 2, 'F32', 'BF16'),
    (2, 32768, 96, 48, 1, 0, 1, 'F32', 'BF16'),
    (2, 32768, 96, 384, 1, 0, 3, 'F32', 'BF16'),
    (2, 32768, 112, 128, 1, 0, 1, 'F32', 'BF16'),
    (2, 32768, 128, 64, 1, 0, 2, 'F32', 'BF16'),
    (2, 32768, 128, 288, 1, 0, 1, 'F32', 'BF16'),
    (2, 32768, 384, 96, 1, 0, 3, 'F32', 'BF16'),
    (2, 8192, 96, 192, 1, 0, 2, 'F32', 'BF16'),
    (2, 8192, 96, 576, 1, 0, 1, 'F32', 'BF16'),
    (2, 8192, 96, 864, 0, 0, 3, 'F32', 'BF16'),
    (2, 8192, 192, 96, 1, 0, 3, 'F32', 'BF16'),
    (2, 8192, 192, 384, 0, 0, 1, 'F32', 'BF16'),
    (2, 8192, 192, 576, 1, 0, 1, 'F32', 'BF16'),
    (2, 8192, 192, 768, 1, 0, 3, 'F32', 'BF16'),
    (2, 8192, 768, 192, 1, 0, 3, 'F32', 'BF16'),
    (2, 2048, 192, 384, 1, 0, 2, 'F32', 'BF16'),
    (2, 2048, 192, 1152, 1, 0, 1, 'F32', 'BF16'),
    (2, 2048, 192, 1728, 0, 0, 3, 'F32', 'BF16'),
    (2, 2048, 384, 192, 1, 0, 3, 'F32', 'BF16'),
    (2, 2048, 384, 768, 0, 0, 1, 'F32', 'BF16'),
    (2, 2048, 384, 1152, 1, 0, 1, 'F32', 'BF16'),
    (2, 2048, 384, 1536, 1, 0, 9, 'F32', 'BF16'),
    (2, 2048, 1536, 384, 1, 0, 9, 'F32', 'BF16'),
    (1, 672, 4, 128, 1, 1, 6, 'F32', 'F32'),
    (1, 672, 4, 132, 1, 1, 2, 'F32', 'F32'),
    (1, 672, 128, 4, 1, 1, 2, 'F32', 'F32'),
    (1, 672, 128, 128, 1, 0, 4, 'F32', 'F32'),
    (1, 672, 128, 132, 1, 1, 2, 'F32', 'F32'),
    (1, 672, 128, 512, 1, 0, 2, 'F32', 'F32'),
    (2, 512, 384, 768, 1, 0, 1, 'F32', 'BF16'),
    (2, 512, 384, 3456, 0, 0, 1, 'F32', 'BF16'),
    (2, 512, 768, 384, 1, 0, 1, 'F32', 'BF16'),
    (2, 512, 768, 1536, 0, 0, 1, 'F32', 'BF16'),
    (2, 512, 768, 3072, 1, 0, 3, 'F32', 'BF16'),
    (2, 512, 3072, 768, 1, 0, 3, 'F32', 'BF16'),
]


def _force(form):
    from keypointfusion_amd import lib as L
    return L.KPF_WGRAD_FORM[form] if form else 0


def _tile(form, p):
    return WF.TILE.get(WF.family(p), (32 * p.vn, 32 * p.vk))


# ----------------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_forms_have_every_kind_of_workgroup():
    from keypointfusion_amd import lib as L
    lib = L.load()
    try:
        for form in list(F32_FORMS) + list(H16_FORMS):
            lib.kpf_conv2d_wgrad_force_form(_force(form))
            for kind in (("f32", "r_bf16") if form in F32_FORMS else ("bf16", "f16")):
                for name in VARIANTS:
                    v = variant(name, kind)
                    p = WF.plan(v)
                    fam = WF.family(p)
                    if form in F32_FORMS:  # the forced tile, the 16-bit products on the 64 x 64 tile only, no shortcut
                        assert (p.vn, p.vk) == F32_FORMS[form] and fam == ("r16" if kind == "r_bf16" and form == "f32_2x2" else "f32"), (form, name, fam, p.vn, p.vk)
                    else:
                        assert fam == form, (form, name, fam)
                    bn, bk = _tile(form, p)
                    assert p.tiles_n == -(-WF.N // bn) and p.tiles_k == -(-v.K // bk)
                    assert WF.N // bn >= 1 and WF.N % bn and v.K // bk >= 1 and v.K % bk, (form, name, bn, bk)  # an interior and a ragged tile in N and in K
                    px = WF.STAGE_PIXELS[fam]
                    stages = -(-v.M // px)
                    assert v.M % px, (form, name)                                                  # a ragged last stage
                    assert p.sps * (p.S - 1) < stages <= p.sps * p.S                                # the splits cover the stages, none is empty
                    assert (p.S == 1) if name in WF.UNSPLIT else (p.S >= 2), (form, name, p.S)
                    assert p.writes_dw == int(v.one and p.S == 1 and not v.trimmed)
                    assert p.ws_floats == p.S * (WF.N * v.K + WF.N)
                    assert v.G * p.ws_floats <= v.G * lib.kpf_conv2d_wgrad_ws_floats(v.M, WF.N, v.K), (form, name)  # the size query covers the forced form
        lib.kpf_conv2d_wgrad_force_form(0)
        # nothing forced: the shortcut of fp32 operands, and the few-pixels rule (`big`) of 16-bit operands selects the unsplit 128-tile kernel
        p = WF.plan(variant("direct", "f32"))
        assert WF.family(p) == "direct" and (p.vn, p.vk, p.S, p.writes_dw) == (2, 2, 1, 1)
        q = L.WgradPlan()
        for groups, M, n, k in ((1, 64, 2048, 2048), (4, 64, 1024, 1024), (1, 77, 2048, 2048)):
            L.check(lib.kpf_conv2d_wgrad_plan(L.KPF_DT_BF16, groups, M, n, k, 1, 0, C.byref(q)))
            assert L.KPF_WGRAD_FAMILY[q.family] == "h16" and q.S == 1 and q.sps == -(-M // 32) and q.writes_dw == 1, (groups, M, n, k)
        L.check(lib.kpf_conv2d_wgrad_plan(L.KPF_DT_BF16, 1, 64, 1024, 1024, 1, 0, C.byref(q)))  # 64 tiles: below the rule
        assert L.KPF_WGRAD_FAMILY[q.family] == "h16s"
        assert lib.kpf_conv2d_wgrad_force_form(7) != 0 and lib.kpf_conv2d_wgrad_force_form(-1) != 0  # unknown forms are refused
        # the forms of the benchmark's training step
        for step, col in (("train128", 7), ("train128_bf16", 8)):
            seen = {}
            for row in sorted(BENCH_SHAPES, key=lambda r: -r[1] * r[2] * r[3] * r[6]):
                groups, M, n, k, one, trimmed, calls = row[:7]
                if row[col] is None:
                    continue
                L.check(lib.kpf_conv2d_wgrad_plan(getattr(L, "KPF_DT_" + row[col]), groups, M, n, k, one, trimmed, C.byref(q)))
                fam = L.KPF_WGRAD_FAMILY[q.family]
                bn, bk = WF.TILE.get(fam, (32 * q.vn, 32 * q.vk))
                key = "%s %dx%d" % (fam, bn, bk)
                seen[key] = seen.get(key, 0) + calls
                print("BENCH %-13s %-12s G=%d M=%-6d N=%-5d K=%-5d %s%s x%-2d -> %-6s tile %3d x %-3d S=%-3d sps=%d" % (
                    step, row[col], groups, M, n, k, "1x1" if one else "kxk", " trimmed" if trimmed else "", calls, fam, bn, bk, q.S, q.sps))
            print("BENCH %-13s calls per form: %s" % (step, dict(sorted(seen.items()))))
            assert sum(seen.values()) == sum(r[6] for r in BENCH_SHAPES if r[col] is not None)
    finally:
        lib.kpf_conv2d_wgrad_force_form(0)


# ----------------------------------------------------------------------------------------------------------------------------------------
# on the MI355X
# ----------------------------------------------------------------------------------------------------------------------------------------
def _held(form, v, dw, db, problems):
    errs = WF.errors(v, dw, db)
    print(WF.line(form, v, errs))
    for what, (ek, ep) in errs.items():
        if not WF.within(ek, ep):
            problems.append("%s %s/%s %s: e_kernel %.3e > 4 * %.3e + %.3e" % (form, v.name, v.kind, what, ek, ep, WF.FLOOR))


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("form", list(F32_FORMS))
def test_f32_tiles(form, name):
    """wgrad_f32_kernel<vn, vk> on fp32 operands, each tile x every variant ("direct" forced is the same shape without the shortcut)."""
    v = variant(name, "f32")
    dw, db, p = WF.run(v, _force(form))
    assert WF.family(p) == "f32" and (p.vn, p.vk) == F32_FORMS[form]
    problems = []
    _held(form, v, dw, db, problems)
    if v.G > 1:  # "fp32 operands also keep their split and summation order (bit-identical results)": the channel-stacked launch against one call per group
        for g in range(v.G):
            dg, bg, pg = WF.run(v, _force(form), group=g)
            assert (pg.S, pg.sps) == (p.S, p.sps)
            assert WF.bits(dw[g], dg[0]) and WF.bits(db[g], bg[0]), "%s %s: group %d differs from its own call" % (form, name, g)
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f32", "r_bf16", "r_f16", "bf16", "f16"])
def test_direct_and_unforced_calls(kind):
    """Nothing forced: every variant gives the bits of the forced call on the form kpf_conv2d_wgrad_plan names, and meets the bound.  fp32 operands over M = 99
    pixels of a 1x1 take the one-workgroup shortcut: the plan says so and the descriptor comes back with kind < 0."""
    from keypointfusion_amd import lib as L
    problems = []
    for name in VARIANTS:
        v = variant(name, kind)
        dw, db, p = WF.run(v, 0, defer=name == "direct")
        fam = WF.family(p)
        if name == "direct":
            assert p.writes_dw == 1 and fam == {"f32": "direct", "r_bf16": "r16", "r_f16": "r16"}.get(kind, "h16s"), (kind, fam)
        _held("auto:" + fam, v, dw, db, problems)
        form = fam if fam in H16_FORMS else [f for f, t in F32_FORMS.items() if t == (p.vn, p.vk)][0]
        fw, fb, fp = WF.run(v, L.KPF_WGRAD_FORM[form])
        assert (fp.S, fp.sps, fp.vn, fp.vk) == (p.S, p.sps, p.vn, p.vk), (name, kind, form)
        if not (WF.bits(dw, fw) and WF.bits(db, fb)):
            problems.append("%s/%s: the unforced call differs from the forced call on %s" % (name, kind, form))
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lin", "k3", "trim"])
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_r16_forms(prec, name):
    """KPF_DT_F32_MMA_BF16 / _F16: wgrad_r16_kernel on the 64 x 64 tile, against the products of the rounded operands; under a forced (4, 4) tile the documented
    fallback, the bits of the fp32 call on that tile."""
    v = variant(name, "r_" + prec)
    dw, db, p = WF.run(v, _force("f32_2x2"))
    assert WF.family(p) == "r16"
    problems = []
    _held("r16", v, dw, db, problems)
    far = float((dw.double() - WF._grads(v.x, v.dy, v, torch.float64)[0]).abs().max() / v.ref_dw.abs().max())
    assert far > 1e-4, far  # (the rounded products are orders of magnitude from the fp32 ones: the 16-bit kernel did run)
    fw, fb, fp = WF.run(v, _force("f32_4x4"))
    assert WF.family(fp) == "f32" and (fp.vn, fp.vk) == (4, 4)
    vf = type(v)(**{**vars(v), "dt_name": "KPF_DT_F32"})
    gw, gb, _ = WF.run(vf, _force("f32_4x4"))
    assert WF.bits(fw, gw) and WF.bits(fb, gb), "KPF_DT_F32_MMA_* on the (4, 4) tile is not the fp32 call"
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("form", H16_FORMS)
def test_h16_forms(form, prec, name):
    """wgrad_h16s_kernel (64-tile, 128-pixel stages) and wgrad_h16_kernel (128-tile) on 16-bit operands, each x every variant: split on M = 286, unsplit on
    "tiny" and "direct".  Channel-stacked groups are held to the bound (each group splits for its share of the chip: same sums, another order)."""
    v = variant(name, prec)
    dw, db, p = WF.run(v, _force(form))
    assert WF.family(p) == form and ((p.S == 1) if name in WF.UNSPLIT else (p.S >= 2))
    problems = []
    _held(form, v, dw, db, problems)
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "f16"])
def test_h16_few_pixels_rule(prec):
    """The unsplit 128-tile kernel as the dispatcher itself reaches it: a 1x1 over M = 77 pixels (two whole stages + 13) with 16 x 16 tiles of 128 x 128."""
    from keypointfusion_amd import lib as L
    lib = L.load()
    d = WF.dev()
    tdt = WF.KINDS[prec][0]
    M, n, k = 77, 2048, 2048
    g = torch.Generator().manual_seed(77)
    x, dy = torch.randn(M, k, generator=g).to(tdt), torch.randn(M, n, generator=g).to(tdt)
    ref = dy.double().t() @ x.double()
    plain = dy.float().t() @ x.float()
    rdb, pdb = dy.double().sum(0), dy.float().sum(0)
    p = L.WgradPlan()
    L.check(lib.kpf_conv2d_wgrad_plan(getattr(L, WF.KINDS[prec][2]), 1, M, n, k, 1, 0, C.byref(p)))
    assert L.KPF_WGRAD_FAMILY[p.family] == "h16" and p.S == 1 and p.writes_dw == 1
    dw, db, ws = WF._canaries(n * k, d), WF._canaries(n, d), WF._canaries(p.ws_floats, d)
    xd, yd = x.to(d), dy.to(d)
    L.check(lib.kpf_conv2d_wgrad(yd.data_ptr(), xd.data_ptr(), getattr(L, WF.KINDS[prec][2]), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), p.ws_floats, 1, M, 1, 1, k, k,
                                 1, 1, n, n, 1, 1, 1, 1, 0, 0, 0, 0, None, torch.cuda.current_stream().cuda_stream), "kpf_conv2d_wgrad")
    torch.cuda.synchronize()
    assert WF._kept(dw[n * k:]) and WF._kept(db[n:]) and WF._kept(ws), "wrote behind dw / db, or into the workspace"
    gw, gb = dw[:n * k].view(torch.float32).cpu().view(n, k), db[:n].view(torch.float32).cpu()
    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())
    for what, got, r, pl in (("dw", gw, ref, plain), ("db", gb, rdb, pdb)):
        den = float(r.abs().max())
        ek, ep = float((got.double() - r).abs().max()) / den, float((pl.double() - r).abs().max()) / den
        print("WGRAD %-8s %-7s %-6s  %s e_kernel %.3e e_plain %.3e" % ("h16:big", "M77", prec, what, ek, ep))
        assert WF.within(ek, ep), (what, ek, ep)


@pytest.mark.gpu
@pytest.mark.parametrize("form,kind,name", [("f32_2x4", "f32", "k3"), ("f32_4x4", "f32", "trim"), ("f32_2x2", "r_bf16", "lin"), ("h16s", "bf16", "k3s2"),
                                            ("h16", "f16", "trim"), ("h16s", "f16", "lin_g2"), ("f32_4x2", "f32", "k3_g2"), ("h16", "bf16", "tiny")])
def test_deferred_reduce_has_the_bits_of_the_immediate_one(form, kind, name):
    """One variant per family (and an unsplit one, whose descriptor says that nothing is pending): a descriptor + kpf_wgrad_reduce_multi against the call's own reduce."""
    v = variant(name, kind)
    dw, db, p = WF.run(v, _force(form))
    ew, eb, ep = WF.run(v, _force(form), defer=True)
    assert (ep.S, ep.sps) == (p.S, p.sps)
    assert WF.bits(dw, ew) and WF.bits(db, eb)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(ENV_FORMS))
def test_environment_selected_forms(setting):
    """The kernels behind the tuning switches, which are read once per process: one fresh child per setting runs lin, k3 and trim in both 16-bit types and prints
    its errors.  A child that dies on a signal, exits without its record or runs out of time has met a GPU fault: that is a finding, not a test to run again."""
    env = dict(os.environ)
    for kv in setting.split():
        key, val = kv.split("=")
        env[key] = val
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgrad_forms_child.py")
    try:
        r = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("GPU FAULT? the child of %s ran out of time: find the cause before running it again" % setting, pytrace=False)
    recs = [ln for ln in r.stdout.splitlines() if ln.startswith("WGRAD_CHILD ")]
    assert r.returncode >= 0, "GPU FAULT: the child of %s died on signal %d\n%s" % (setting, -r.returncode, r.stderr[-2000:])
    assert r.returncode == 0 or recs, "GPU FAULT? the child of %s exited with %d and no record\n%s" % (setting, r.returncode, r.stderr[-2000:])
    assert r.returncode == 0 and len(recs) == 1, "the child of %s failed (%d)\n%s\n%s" % (setting, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = json.loads(recs[0][len("WGRAD_CHILD "):])
    assert sorted((x["variant"], x["kind"]) for x in rows) == sorted((n, k) for n in ("lin", "k3", "trim") for k in ("bf16", "f16"))
    problems = []
    for x in rows:
        assert x["family"] == ENV_FORMS[setting], (setting, x)  # the switch was seen
        v = variant(x["variant"], x["kind"])
        errs = {w: tuple(x[w]) for w in ("dw", "db")}
        print(WF.line("env:" + x["family"], v, errs) + "  " + setting)
        problems += ["%s %s/%s %s: e_kernel %.3e > 4 * %.3e + %.3e" % (setting, x["variant"], x["kind"], w, e[0], e[1], WF.FLOOR) for w, e in errs.items() if not WF.within(*e)]
    assert not problems, "\n".join(problems)

