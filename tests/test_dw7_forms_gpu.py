"""Every form of the depthwise 7x7 family — kpf_dwconv7_ln_f32 / _split_f32 / _h16, kpf_dwconv7_f32 / _add_f32 (csrc/kpf_elem.hip) and kpf_dwconv7_wgrad (part (2) /
(2b) of csrc/kpf_wgrad.hip) — on small shapes that reach it by the dispatcher's own rules, pinned to torch's float64 conv2d(groups = C) + layer_norm (or conv2d
backward) on the CPU.  The sibling of test_igemm_tiles_gpu.py and test_wgrad_forms_gpu.py.  Which kernel a launch takes follows from how well it fills the chip
and from tuning switches read once per process; kpf_dwconv7_plan asks the launchers' own selection functions, so the tables below are checked, not believed.
Shapes, operands, references and the guarded calls: dw7_forms.py.

What is asserted:
 1. accuracy.  fp32: e_kernel <= 4 * e_plain + 8 * 2^-24, both relative to max|ref64|, e_plain = the same operation in plain fp32 torch on the CPU.  Split output:
    the same on from_split(y), plus what a to_split / from_split round trip does to the float64 reference itself.  16-bit storage:
    igemm_bounds.h16_excess(.., "rounding") against float64 on the activation as stored.
 2. guards: every operand, output and the workspace (exactly the size the plan names) sits between guards of a quiet NaN with a payload, outputs and workspace
    start as that NaN: the guards keep their bits and the output is finite.
 3. bits: the weight gradient twice; the four (PX, rows) forms of dwconv7_kernel; PX 4 against PX 8 of the two-launch path.  Between families only a line says
    whether the bits agree.
 4. the forms behind KPF_DW7_MIN_BLOCKS, KPF_DW7_PX, KPF_DW7_ROWS, KPF_DW7_WGRAD_LDS, KPF_DW7_TARGET, KPF_DW7_MINROWS, KPF_DW_UNFUSED, KPF_DW_PX, KPF_DW_WIDE:
    one fresh child per setting (dw7_forms_child.py), held to 1 and 2 — each runs its cases as the dispatcher sends them under the switch.
test_shape_table_reaches_every_form (no GPU) proves through the plan query that the table reaches every family and parameter it claims and pins the rule at the
benchmark's shapes.  One line per comparison ("DW7 op family case type e_kernel e_plain"); profiles/dw7_form_errors.txt is one run on the MI355X.

Where the query disagreed with the plan of this suite: KPF_DW7_TARGET=3 KPF_DW7_MINROWS=1 gives ceil(3 / channel blocks) chunks (three of five rows on the H = 7
shapes: chunks that start at rows 5 and 10, inside both images), not one-row chunks; those are what KPF_DW7_MINROWS=1 alone gives, which runs as a setting of
its own.  In split form the maps below 8 x 8 take the two-launch path, not the tiny fused kernel (which has no split output).

What this suite found: in 16-bit storage the two-launch path rounded the un-normalised map to 16 bits between its launches; (2, 9, 13, 1056) in bf16 came back
with e_kernel 7.1e-3 and h16_excess +2.0 (the bound is <= 0).  16-bit storage now takes the fused kernel with the fp32 tile on those shapes (C > 1024, or
behind KPF_DW_UNFUSED / KPF_DW_WIDE=0); of the models here only ConvNeXt-L's last stage (C = 1536) on maps of 8 x 8 and larger took that path."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import dw7_forms as DF
from dw7_forms import LN_CASES, TRAIN_CASES, WGRAD_CASES

# the form the dispatcher gives each case with no switch set (dw7_forms.form); split: where it differs from f32
LN_FORMS = {
    "tile96": "tile<3,8>", "tile128": "tile<4,8>", "tile192": "tile<6,4>",
    "wave40": "wave<32>", "wave96": "wave<32>", "wave128": "wave<32>", "wave136": "wave<64>", "wave192": "wave<64>", "wave256": "wave<64>",
    "wide320": "wide<128,1>", "wide512": "wide<128,1>", "wide640": "wide<192,1>", "wide768": "wide<192,1>", "wide800": "wide<256,1>", "wide1024": "wide<256,1>",
    "wide320r2": "wide<128,2>", "two1056": "two<8,glb>",
    "tiny40": "tiny<1,64>", "tiny96": "tiny<1,64>", "tiny768": "tiny<1,192>", "tiny1056": "tiny<1,320>", "tiny2048": "tiny<1,512>",
}
LN_SPLIT_FORMS = {"tiny96": "two<8,lds>", "tiny768": "two<8,glb>", "tiny1056": "two<8,glb>", "tiny2048": "two<8,glb>"}
CONV_FORMS = {"c8": "conv<4,1,lds>", "c100": "conv<4,1,lds>", "c248": "conv<4,1,lds>", "c252": "conv<4,1,glb>", "m4x4": "conv<4,1,lds>", "m2x3": "conv<4,1,lds>",
              "m1x1": "conv<4,1,lds>"}
WGRAD_FORMS = {  # <channel quads per workgroup, chunks x rows per chunk>
    "c8": "lds<2,4x4>", "c100": "lds<16,4x4>", "c248": "lds<16,4x4>", "c252": "lds<16,4x4>", "m4x4": "lds<32,2x4>", "m2x3": "lds<2,1x2>", "m1x1": "lds<2,1x1>",
    "w20": "lds<8,6x4>", "w70": "lds<4,1x3>", "q32": "lds<32,4x4>", "w296": "reg<0,2x1>"}
LN_H16_FORMS = {"two1056": "tiny<1,320>"}  # 16-bit storage has no two-launch path (its intermediate map would be rounded): the fused kernel with the fp32 tile


def _ln_form(name, kind):
    return {"split": LN_SPLIT_FORMS, "bf16": LN_H16_FORMS, "f16": LN_H16_FORMS}.get(kind, {}).get(name, LN_FORMS[name])


def _two_launch(r, px, taps_lds=None):
    """a row of a child whose setting sends the case to the two-launch path (fp32 storage) or, in 16-bit storage, to the fused kernel behind it"""
    if r["kind"] in ("bf16", "f16"):
        return r["plan"]["family"] == "tiny"
    return r["plan"]["family"] == "two_launch" and r["plan"]["px"] == px and (taps_lds is None or r["plan"]["taps_lds"] == taps_lds)


RAISED_LDS = ("m4x4", "q32")  # 32-quad blocks: 66.5 KB

# setting -> (the child's cases, what every row's plan must show under it: the switch was seen)
SETTINGS = {
    "KPF_DW7_MIN_BLOCKS=1": ("fwd", lambda r: (r["plan"]["px"], r["plan"]["rows"]) == ((8 if WGRAD_CASES[r["case"]][2] > 4 else 4), 2)),
    "KPF_DW7_PX=8 KPF_DW7_ROWS=1": ("fwd", lambda r: (r["plan"]["px"], r["plan"]["rows"]) == (8, 1)),
    "KPF_DW7_PX=4 KPF_DW7_ROWS=2": ("fwd", lambda r: (r["plan"]["px"], r["plan"]["rows"]) == (4, 2)),
    "KPF_DW7_WGRAD_LDS=0": ("wgrad", lambda r: r["plan"]["family"] == "wgrad_reg"),
    "KPF_DW7_TARGET=3 KPF_DW7_MINROWS=1": ("wgrad", lambda r: r["plan"]["family"] == "wgrad_reg" or (
        r["plan"]["S"] <= 3 and (r["case"] != "c8" or (r["plan"]["S"], r["plan"]["rows_per_chunk"]) == (3, 5)))),
    "KPF_DW7_MINROWS=1": ("wgrad", lambda r: r["plan"]["family"] == "wgrad_reg" or r["plan"]["rows_per_chunk"] == 1),
    "KPF_DW_UNFUSED=1": ("ln_wave", lambda r: _two_launch(r, 8)),
    "KPF_DW_UNFUSED=1 KPF_DW_PX=4": ("ln_wave", lambda r: _two_launch(r, 4)),
    "KPF_DW_WIDE=0": ("ln_wide", lambda r: _two_launch(r, 8, 0)),
}
SAME_BITS_AS_DEFAULT = ("KPF_DW7_MIN_BLOCKS=1", "KPF_DW7_PX=8 KPF_DW7_ROWS=1", "KPF_DW7_PX=4 KPF_DW7_ROWS=2")  # the same fmaf sequence per output


# ----------------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_shape_table_reaches_every_form():
    from keypointfusion_amd import lib as L
    lib = L.load()
    assert set(LN_FORMS) == set(LN_CASES) and set(CONV_FORMS) == set(TRAIN_CASES) and set(WGRAD_FORMS) == set(WGRAD_CASES)
    seen = set()
    for name, shape in LN_CASES.items():
        Bn, H, W, Cc, _ = shape
        for kind in DF.ln_kinds(name):
            p = DF.plan("ln", shape, kind)
            assert DF.form(p) == _ln_form(name, kind), (name, kind, DF.form(p))
            seen.add((DF.form(p), kind))
            fam = DF.family(p)
            if fam == "tile":  # an interior and a ragged tile in both directions; with 7 taps every interior tile edge is crossed by a halo
                tx = 4 * p.px
                assert p.rows == 8 and H // 8 >= 2 and H % 8 and W // tx >= 1 and W % tx and p.blocks == Bn * -(-H // 8) * -(-W // tx) and p.nchk * 32 == Cc
            if fam == "wave":  # whole strips and ragged ones in both directions; 40 and 136 channels leave idle lanes in the LayerNorm shuffles
                assert H % 2 and W % 8 and W > 8 and p.lds_bytes == 49 * Cc * 4 and Cc // 4 <= p.lg and (p.lg == 32 or Cc // 4 > 32)
                assert p.blocks == -(-Bn * -(-H // 2) * -(-W // 8) * p.lg // 256)
            if fam == "wide":
                assert p.nt >= Cc // 4 and (p.nt == 128 or Cc // 4 > p.nt - 64) and W % 8 and p.blocks == Bn * -(-H // p.rows) * -(-W // 8)
                assert (p.rows == 2) == (Bn * -(-H // 2) * -(-W // 8) >= 256) and (p.rows == 1 or H % 2)
            if fam == "two_launch":
                assert p.taps_lds == int(49 * Cc * 4 <= 48 * 1024) and p.lds_bytes == (49 * Cc * 4 if p.taps_lds else 0)
            if fam == "tiny":
                assert (H * W < 64 or kind in ("bf16", "f16")) and p.lds_bytes == p.S * 8 * Cc * 4 <= 64 * 1024 and p.nt % 64 == 0 and Cc // 4 <= p.nt <= 512 and p.blocks == Bn * H * -(-W // (8 * p.S))
    for f in set(LN_FORMS.values()):  # every form in every storage type it supports: the tiny kernel has no split output, the two-launch path no 16-bit storage
        for kind in DF.KINDS:
            assert (f, kind) in seen or (kind == "split" and f.startswith("tiny")) or (kind in ("bf16", "f16") and f.startswith("two")), (f, kind)
    assert {"two<8,lds>", "two<8,glb>"} <= {f for f, k in seen if k == "split"}
    assert sum(1 for n in LN_CASES if LN_CASES[n][3] // 4 < DF.plan("ln", LN_CASES[n]).lg) >= 4  # lane groups with idle lanes, both widths
    for fam in ("tile", "wave", "wide", "two", "tiny"):
        assert any(LN_CASES[n][4] for n in LN_CASES if LN_FORMS[n].startswith(fam)), fam  # a case with |mean| >> sigma in every family

    for name, shape in TRAIN_CASES.items():
        p = DF.plan("fwd", shape)
        assert DF.form(p) == CONV_FORMS[name], (name, DF.form(p))
        assert p.taps_lds == int(shape[3] <= 248) and p.blocks == -(-shape[0] * -(-shape[1] // p.rows) * -(-shape[2] // p.px) * (shape[3] // 4) // 256)
    for name, shape in WGRAD_CASES.items():
        Bn, H, W, Cc = shape
        p = DF.plan("wgrad", shape)
        assert DF.form(p) == WGRAD_FORMS[name], (name, DF.form(p))
        assert p.raise_lds == int(name in RAISED_LDS) and (p.lds_bytes > 64 * 1024) == bool(p.raise_lds)
        assert p.S == -(-Bn * H // p.rows_per_chunk) and p.ws_floats == p.S * 50 * Cc <= lib.kpf_dwconv7_wgrad_ws_floats(Bn, H, Cc)
        if H == 7 and Bn == 2:  # four-row chunks: the second starts at row 4 of the first image and runs into the second image
            assert p.rows_per_chunk == 4 and H % p.rows_per_chunk and p.S == 4
    assert DF.plan("wgrad", (1, 2, 288, 8)).family == L.KPF_DW7_FAMILY.index("wgrad_lds")  # 36 segments: the widest map of the LDS kernel
    assert DF.plan("wgrad", (1, 2, 289, 8)).family == L.KPF_DW7_FAMILY.index("wgrad_reg")
    assert DF.form(DF.plan("wgrad", (1, 2, 150, 8))).startswith("lds<1,")                  # (test_kernels_train_gpu.py: its widest map is still the LDS kernel)

    # the rule at the benchmark's shapes: ConvNeXt-T on 128 x 128 crops, stage maps 32 x 32 x 96 ... 4 x 4 x 768
    stages = lambda Bn: [(Bn, 32, 32, 96), (Bn, 16, 16, 192), (Bn, 8, 8, 384), (Bn, 4, 4, 768)]
    assert DF.form(DF.plan("fwd", (128, 32, 32, 96))) == "conv<8,2,lds>" and DF.plan("fwd", (128, 32, 32, 96)).blocks == 768
    assert DF.form(DF.plan("fwd", (32, 8, 8, 384))) == "conv<4,1,glb>"
    assert [DF.form(DF.plan("fwd", s)) for s in stages(32)] == ["conv<4,1,lds>", "conv<4,1,lds>", "conv<4,1,glb>", "conv<4,1,glb>"]
    assert [DF.form(DF.plan("fwd", s)) for s in stages(64)] == ["conv<4,2,lds>", "conv<4,1,lds>", "conv<4,1,glb>", "conv<4,1,glb>"]
    assert [DF.form(DF.plan("fwd", s)) for s in stages(128)] == ["conv<8,2,lds>", "conv<4,2,lds>", "conv<4,1,glb>", "conv<4,1,glb>"]
    assert DF.form(DF.plan("fwd", (8, 32, 32, 192))) == "conv<4,1,lds>"  # the largest shape of test_kernels_train_gpu.py: 96 workgroups in the widest form
    for Bn in (32, 64, 128):
        for s in stages(Bn):
            pw, pl = DF.plan("wgrad", s), DF.plan("ln", s)
            assert DF.family(pw) == "wgrad_lds" and pw.raise_lds == int(s[3] >= 384) and DF.family(pl) == ("tile" if s[1] >= 16 else "wide")
            print("BENCH B=%-3d %-18s fwd %-14s wgrad %-14s inference %s" % (Bn, "x".join(map(str, s[1:])), DF.form(DF.plan("fwd", s)), DF.form(pw), DF.form(pl)))

    # what the entry points refuse the query refuses; an unknown op or type is refused
    q = L.Dw7Plan()
    for args in ((0, 0, 0, 1, 4, 4, 6), (0, 0, 0, 1, 4, 4, 2052), (0, 0, 1, 1, 4, 4, 40), (0, 1, 1, 1, 4, 4, 96), (1, 1, 0, 1, 4, 4, 96), (2, 0, 1, 1, 4, 4, 96),
                 (3, 0, 0, 1, 4, 4, 96), (0, 3, 0, 1, 4, 4, 96), (1, 0, 0, 0, 4, 4, 96)):
        assert lib.kpf_dwconv7_plan(*args, C.byref(q)) != 0, args


# ----------------------------------------------------------------------------------------------------------------------------------------
# on the MI355X
# ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _default_ln(name, kind):
    return DF.run_ln(name, kind)


@functools.lru_cache(maxsize=None)
def _default_conv(name, op):
    return DF.run_conv(name, op)


@functools.lru_cache(maxsize=None)
def _default_wgrad(name):
    return DF.run_wgrad(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [(n, k) for n in LN_CASES for k in DF.ln_kinds(n)])
def test_inference_forms(name, kind):
    """kpf_dwconv7_ln_f32 / _split_f32 / _h16: every family x every storage type it supports, as the dispatcher sends the shape."""
    y, p = _default_ln(name, kind)
    assert DF.form(p) == _ln_form(name, kind)
    f = DF.ln_figures(DF.ln_case(name, kind), kind, y)
    print(DF.line("ln", DF.form(p), name, kind, f))
    assert not DF.misses(f), "%s/%s %s: %s" % (name, kind, DF.form(p), DF.misses(f))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRAIN_CASES))
def test_training_conv_forms(name):
    """kpf_dwconv7_f32 forward, the data gradient (the same kernel on dy with mirrored taps) and kpf_dwconv7_add_f32 with the skip path's gradient."""
    v = DF.train_case(name)
    problems = []
    for op in ("fwd", "dgrad", "dgrad_add"):
        y, p = _default_conv(name, op)
        assert DF.form(p) == CONV_FORMS[name]
        ek, ep = DF.rel_errors(y, v.ref[op], v.plain[op])
        f = {"e_kernel": ek, "e_plain": ep}
        print(DF.line(op, DF.form(p), name, "f32", f))
        if DF.misses(f):
            problems.append("%s %s: %s" % (op, name, DF.misses(f)))
    assert not problems, "\n".join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_weight_gradient_forms(name):
    """kpf_dwconv7_wgrad: dw and db, the LDS kernel in every channel-block size (with and without the raised limit) and the register-window kernel that a map of
    296 columns takes by shape alone; twice, same bits (fixed-order sums)."""
    v = DF.train_case(name)
    dw, db, p = _default_wgrad(name)
    assert DF.form(p) == WGRAD_FORMS[name]
    dw2, db2, _ = DF.run_wgrad(name)
    assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32)), "two runs differ in their bits"
    problems = []
    for what, got in (("dw", dw), ("db", db)):
        ek, ep = DF.rel_errors(got, v.ref[what], v.plain[what])
        f = {"e_kernel": ek, "e_plain": ep}
        print(DF.line(what, DF.form(p), name, "f32", f))
        if DF.misses(f):
            problems.append("%s %s: %s" % (what, name, DF.misses(f)))
    assert not problems, "\n".join(problems)


@functools.lru_cache(maxsize=None)
def _child(setting):
    """one fresh process under `setting` -> its rows.  A child that dies on a signal, exits without its record or runs out of time has met a GPU fault: that is a
    finding to understand from the code, not a test to run again."""
    env = dict(os.environ)
    for kv in setting.split():
        key, val = kv.split("=")
        env[key] = val
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dw7_forms_child.py")
    try:
        r = subprocess.run([sys.executable, child, SETTINGS[setting][0]], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("GPU FAULT? the child of %s ran out of time: find the cause before running it again" % setting, pytrace=False)
    recs = [ln for ln in r.stdout.splitlines() if ln.startswith("DW7_CHILD ")]
    assert r.returncode >= 0, "GPU FAULT: the child of %s died on signal %d\n%s" % (setting, -r.returncode, r.stderr[-2000:])
    assert r.returncode == 0 or recs, "GPU FAULT? the child of %s exited with %d and no record\n%s" % (setting, r.returncode, r.stderr[-2000:])
    assert r.returncode == 0 and len(recs) == 1, "the child of %s failed (%d)\n%s\n%s" % (setting, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(recs[0][len("DW7_CHILD "):])


def _default_bits(row):
    """(CRC, form) of the same comparison in this process, where no switch is set"""
    if row["op"] == "ln":
        y, p = _default_ln(row["case"], row["kind"])
    elif row["op"] in ("dw", "db"):
        dw, db, p = _default_wgrad(row["case"])
        y = dw if row["op"] == "dw" else db
    else:
        y, p = _default_conv(row["case"], row["op"])
    return DF.crc(y), DF.form(p)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_switch_selected_forms(setting):
    """The kernels behind the tuning switches, read once per process: one fresh child per setting runs the cases the switch bears on, nothing forced, and prints
    its plans, figures and CRCs.  Here: the switch was seen (the plan query of the child names the form the setting asks for), the bounds, and the bits where
    the arithmetic is the same fmaf sequence per output."""
    group, seen = SETTINGS[setting]
    rows = _child(setting)
    want = {"fwd": [(op, n, "f32") for n in TRAIN_CASES for op in ("fwd", "dgrad", "dgrad_add")],
            "wgrad": [(op, n, "f32") for n in WGRAD_CASES for op in ("dw", "db")]}.get(group) or [
                ("ln", n, k) for n in LN_CASES if n.startswith(group[3:]) for k in DF.ln_kinds(n)]
    assert sorted((r["op"], r["case"], r["kind"]) for r in rows) == sorted(want)
    problems = []
    for r in rows:
        assert seen(r), (setting, r["case"], r["plan"])  # the switch was seen
        crc0, form0 = _default_bits(r)
        same = crc0 == r["crc"]
        print(DF.line(r["op"], r["plan"]["form"], r["case"], r["kind"], r["fig"], "%s  bits %s %s" % (setting, "agree with" if same else "differ from", form0)))
        if DF.misses(r["fig"]):
            problems.append("%s %s %s/%s %s: %s" % (setting, r["op"], r["case"], r["kind"], r["plan"]["form"], DF.misses(r["fig"])))
        if setting in SAME_BITS_AS_DEFAULT and not same:
            problems.append("%s %s %s: %s differs in its bits from %s" % (setting, r["op"], r["case"], r["plan"]["form"], form0))
    if setting == "KPF_DW_UNFUSED=1 KPF_DW_PX=4":  # the same fmaf sequence and the same LayerNorm launch behind it
        other = {(r["case"], r["kind"]): r for r in _child("KPF_DW_UNFUSED=1")}
        for r in rows:
            o = other[(r["case"], r["kind"])]
            assert (o["plan"]["px"], r["plan"]["px"]) == (8, 4) or r["kind"] in ("bf16", "f16")
            if o["crc"] != r["crc"]:
                problems.append("two-launch %s/%s: PX 4 differs in its bits from PX 8" % (r["case"], r["kind"]))
    assert not problems, "\n".join(problems)
