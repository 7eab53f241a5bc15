"""Training augmentation by the dataset protocol on the device (DevicePreprocessor.prepare_augmented on kpf_prep_aug_draw + kpf_prep_augment_u16 +
kpf_prep_pcl_sample) against the host path it reproduces (keypointfusion_amd/preprocess.py::prepare_augmented, itself pinned to the reference's training
items by tests/test_prep_augment_host.py), on the frames of tests/annot_cases.py, every mode mixed inside one launch.

The parameters are made on the host and uploaded, so everything is BIT-EQUAL to prepare_augmented: img, img_rgb, joint, joint_img, center, M, M64, cube,
cube64, com, cam_para, the base crop's bounds, aug_status and pcl_count; candidate points within 2.4e-7 and sampled rows bit-equal to candidates[pcl_index]
(the bounds of tests/test_prep_annot_gpu.py).  The drawn parameters equal the host twin bit for bit except rot_cs, which is within 4 ulp of NumPy's (the
accuracy OpenCL requires of double sin / cos, which the device library states it meets)."""
import math

import numpy as np
import pytest
import torch

import annot_cases as AC
import augment_cases as GC
import prep_cases as PC
from keypointfusion_amd import preprocess as P

pytestmark = pytest.mark.gpu
BIT_EQUAL = ("img", "img_rgb", "M", "M64", "center", "com", "cube", "cube64", "cam_para", "joint", "joint_img")
FRAMES = ("right", "left", "corner", "left_edge", "fx_ne_fy", "wall", "given", "empty")
_HOST = {}


def _dev():
    return torch.device("cuda:0")


def _inputs(name):
    """synth()'s tuple with the centre from the joints (the centre is given or not for a whole launch; `given` is covered by its own batch below)."""
    rgb, depth, joints_mm, cam, mirror, center = AC.synth(name)
    if name == "hd_left":
        (x0, y0), (Hs, Ws) = AC.HD_WINDOW
        rgb, depth = PC.embed(rgb[y0:y0 + Hs, x0:x0 + Ws], depth[y0:y0 + Hs, x0:x0 + Ws], (x0, y0), depth.shape)
    return rgb, depth, joints_mm, cam, mirror, None


def _aug_key(aug):
    return tuple((k, np.asarray(v, np.float64).tobytes()) for k, v in sorted(aug.items()) if v is not None)


def _host(ins_key, ins, aug, S=128, n=1024):
    key = (ins_key, _aug_key(aug), S, n)
    if key not in _HOST:  # computed once, shared by the tests, never modified
        _HOST[key] = GC.host_record(ins, aug, S, n)
    return _HOST[key]


def _t(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev()) if dt is None else torch.tensor(a, dtype=dt, device=_dev())


def _batch(items, augs, seeds):
    kw = dict(rgb=_t(np.stack([i[0] for i in items])), depth=_t(np.stack([i[1] for i in items])), joints_mm=_t(np.stack([i[2] for i in items])),
              cam=_t(np.stack([i[3] for i in items])), seed=_t(list(seeds), torch.int64), mirror=_t(np.array([i[4] for i in items], np.uint8)),
              aug={k: _t(v) for k, v in GC.stack(augs).items()})
    if items[0][5] is not None:
        kw["center_xyz"] = _t(np.stack([i[5] for i in items]))
    return kw


def _cpu(prep):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in prep.items() if isinstance(v, torch.Tensor)}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_sample(d, b, h, n=1024):
    assert np.array_equal(d["bounds"][b, :4], h["bounds"]) and np.array_equal(d["bounds"][b, 4:], h["sz"])
    for k in BIT_EQUAL:
        assert _same_bits(d[k][b], h[k]), (k, d[k][b], h[k])
    assert int(d["aug_status"][b]) == h["aug_status"], (int(d["aug_status"][b]), h["aug_status"])
    N = len(h["candidates"])
    assert int(d["pcl_count"][b]) == N
    cand = d["candidates"][b, :N]
    idx, pcl = d["pcl_index"][b], d["pcl"][b]
    if N == 0:
        assert not pcl.any() and (idx == -1).all()
        return
    err = float(np.abs(cand.astype(np.float64) - h["candidates"]).max())
    print("candidates %d, max deviation %.3g" % (N, err))
    assert err <= 2.4e-7
    assert idx.min() >= 0 and idx.max() < N
    assert np.array_equal(pcl.view(np.int32), cand[idx].view(np.int32))
    mult = np.bincount(idx, minlength=N)
    if N >= n:
        assert mult.max() == 1
    else:
        q, r = divmod(n, N)
        assert mult.min() >= q and mult.max() <= q + 1 and int((mult == q + 1).sum()) == r


def _assert_equal(a, c, what=""):
    assert set(a) == set(c)
    for k in a:
        x, y = a[k], c[k]
        if k == "candidates":
            for b in range(len(x)):
                N = int(a["pcl_count"][b])
                assert _same_bits(x[b, :N], y[b, :N]), (what, k, b)
        else:
            assert _same_bits(x, y), (what, k)


def _mixed(B, seed, color=False):
    """B (frame name, draw) pairs: frames and modes interleaved so that every mode meets right and left hands, padding and letterboxing."""
    g = np.random.RandomState(seed)
    names = [n for n in FRAMES if n != "given"]
    return [(names[(3 * i + i // 4) % len(names)], GC.draw(g, i % 4, color and i % 3 == 0)) for i in range(B)]


@pytest.fixture(scope="module")
def pre():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    return DevicePreprocessor(img_size=128, sample_num=1024, cube=AC.CUBE, debug_candidates=True)


@pytest.mark.parametrize("B", [8, 32])
def test_mixed_batches_match_prepare_augmented(pre, B):
    if B == 8:  # four modes x right / left hand
        g = np.random.RandomState(1)
        pairs = [(n, GC.draw(g, m)) for m in range(4) for n in ("right", "left")]
    else:
        pairs = _mixed(32, 2, color=True)
    d = _cpu(pre.prepare_augmented(**_batch([_inputs(n) for n, _ in pairs], [a for _, a in pairs], range(100, 100 + B))))
    for b, (name, aug) in enumerate(pairs):
        print(B, b, name, P.AUG_MODES[aug["mode"]])
        _check_sample(d, b, _host(name, _inputs(name), aug))
    status = d["aug_status"]
    assert (status[[a["mode"] == 3 for _, a in pairs]] == 0).all() and (status & 2 == 0).all() and (status == 1).sum() >= B // 2


def test_given_centre_with_colour(pre):
    """HO3D's item: a given centre (joints used as they are) and the colour scale, in all four modes."""
    g = np.random.RandomState(3)
    ins = AC.synth("given")
    augs = [GC.draw(g, m, color=True) for m in range(4)]
    d = _cpu(pre.prepare_augmented(**_batch([ins] * 4, augs, range(4))))
    for b, aug in enumerate(augs):
        _check_sample(d, b, _host("given*", ins, aug))
    assert not _same_bits(d["img_rgb"][3], _host("given*", ins, dict(augs[3], color=None))["img_rgb"])  # the colour scale acts in mode none too


def test_crop_size_64_with_512_samples():
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    pre64 = DevicePreprocessor(img_size=64, sample_num=512, cube=AC.CUBE, debug_candidates=True)
    pairs = _mixed(8, 4)
    d = _cpu(pre64.prepare_augmented(**_batch([_inputs(n) for n, _ in pairs], [a for _, a in pairs], range(8))))
    for b, (name, aug) in enumerate(pairs):
        _check_sample(d, b, _host(name, _inputs(name), aug, 64, 512), n=512)


def test_results_do_not_depend_on_the_batch_and_replay_from_a_graph():
    """One (frame, annotation, draw, seed) alone and at positions 0, 13 and 31 of a B = 32 batch: every output bit-identical; two runs bit-identical; a
    captured and replayed graph equals the eager run."""
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    pre = DevicePreprocessor(cube=AC.CUBE, debug_candidates=True)
    pairs = _mixed(32, 5)
    g = np.random.RandomState(6)
    for pos, name, mode in ((0, "left_edge", 0), (13, "corner", 1), (31, "left", 2)):
        pairs[pos] = (name, GC.draw(g, mode))
    seeds = [7 + i for i in range(32)]
    items, augs = [_inputs(n) for n, _ in pairs], [a for _, a in pairs]
    kw = _batch(items, augs, seeds)
    big = _cpu(pre.prepare_augmented(**kw))
    _assert_equal(big, _cpu(pre.prepare_augmented(**kw)), "run to run")
    for pos in (0, 13, 31):
        one = _cpu(pre.prepare_augmented(**_batch([items[pos]], [augs[pos]], [seeds[pos]])))
        _assert_equal(one, {k: v[pos:pos + 1] for k, v in big.items()}, pairs[pos][0])
        _check_sample(big, pos, _host(pairs[pos][0], items[pos], augs[pos]))
    # the same batch from a captured graph whose static inputs held another batch at capture time
    pre_g = DevicePreprocessor(cube=AC.CUBE, debug_candidates=True)
    other = _mixed(32, 8)
    static = _batch([_inputs(n) for n, _ in other], [a for _, a in other], range(32))
    dev = _dev()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        pre_g.prepare_augmented(**static)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pre_g.prepare_augmented(**static)
    for k, v in kw.items():
        if k == "aug":
            for kk in v:
                static["aug"][kk].copy_(v[kk])
        else:
            static[k].copy_(v)
    graph.replay()
    _assert_equal(_cpu(out), big, "graph")


def test_a_window_of_the_frame_equals_the_whole_frame_mirrored(pre):
    """hd_left (1080 x 1920, a left hand) uploaded as HD_WINDOW with origin / frame_size against the whole frame, in modes rot and com."""
    g = np.random.RandomState(9)
    rgb, depth, joints_mm, cam, mirror, _ = ins = _inputs("hd_left")
    assert mirror
    (x0, y0), (Hs, Ws) = AC.HD_WINDOW
    augs = [GC.draw(g, 0), GC.draw(g, 1)]
    whole = _cpu(pre.prepare_augmented(**_batch([ins] * 2, augs, [5, 6])))
    win_item = (np.ascontiguousarray(rgb[y0:y0 + Hs, x0:x0 + Ws]), np.ascontiguousarray(depth[y0:y0 + Hs, x0:x0 + Ws]), joints_mm, cam, True, None)
    win = _cpu(pre.prepare_augmented(**_batch([win_item] * 2, augs, [5, 6]), origin=(x0, y0), frame_size=depth.shape))
    _assert_equal(win, whole, "window")
    for b in range(2):
        _check_sample(whole, b, _host("hd_left", ins, augs[b]))
    assert int(whole["pcl_count"][0]) > 500 and (whole["aug_status"] == 1).all()


def test_early_exits_mode_none_and_the_all_zero_crop(pre):
    g = np.random.RandomState(10)
    z3 = np.zeros(3)
    base = GC.draw(g, 3)
    pairs = [("right", dict(base, mode=1, off=z3)), ("left", dict(base, mode=0, rot=0.0, rot_cs=(1.0, 0.0))), ("corner", dict(base, mode=2, sc=1.0)),
             ("fx_ne_fy", dict(base, mode=3)), ("empty", dict(base, mode=0)), ("empty", dict(base, mode=1)), ("empty", dict(base, mode=2)),
             ("left", dict(base, mode=0, rot=360.0, rot_cs=P._rot_cs(360.0)))]
    d = _cpu(pre.prepare_augmented(**_batch([_inputs(n) for n, _ in pairs], [a for _, a in pairs], range(8))))
    for b, (name, aug) in enumerate(pairs):
        _check_sample(d, b, _host(name, _inputs(name), aug))
    assert d["aug_status"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    for b in range(4):  # an early exit is mode none: the geometry and both images of the unaugmented item
        h = _host(pairs[b][0], _inputs(pairs[b][0]), dict(base, mode=3))
        assert all(_same_bits(d[k][b], h[k]) for k in BIT_EQUAL)
    none = _host("empty", _inputs("empty"), dict(base, mode=3))
    for b in (4, 5, 6):  # the all-zero crop: depth, labels and geometry stay, RGB is warped
        assert all(_same_bits(d[k][b], none[k]) for k in BIT_EQUAL if k != "img_rgb") and not _same_bits(d["img_rgb"][b], none["img_rgb"])


def test_refused_parameters_set_the_status_and_give_mode_none(pre):
    """A NaN rot, sc = 0 and offsets no crop can follow are valid inputs with a defined result: aug_status bit 1 and the outputs of mode none."""
    g = np.random.RandomState(11)
    base = GC.draw(g, 3)
    nan = float("nan")
    pairs = [("right", dict(base, mode=0, rot=nan, rot_cs=(nan, nan))), ("left", dict(base, mode=2, sc=0.0)), ("corner", dict(base, mode=1, off=np.array([nan, 0, 0]))),
             ("right", dict(base, mode=3))]
    # finite offsets that take the centre into the camera plane, a hair in front of it (valid: a huge crop), and out of every range
    depth_mm = float(_host("right", _inputs("right"), dict(base, mode=3))["center"][2])
    pairs += [("right", dict(base, mode=1, off=np.array([0.0, 0.0, -depth_mm]))), ("right", dict(base, mode=1, off=np.array([0.0, 0.0, -depth_mm + 1e-3]))),
              ("right", dict(base, mode=1, off=np.array([1e300, 0.0, 0.0]))), ("left", dict(base, mode=1, off=np.array([0.0, 0.0, 1e30])))]
    d = _cpu(pre.prepare_augmented(**_batch([_inputs(n) for n, _ in pairs], [a for _, a in pairs], range(8))))
    assert d["aug_status"].tolist() == [2, 2, 2, 0, 2, 1, 2, 2]
    for b, (name, aug) in enumerate(pairs):
        _check_sample(d, b, _host(name, _inputs(name), aug))
        if b != 5:
            h = _host(name, _inputs(name), dict(base, mode=3))
            assert all(_same_bits(d[k][b], h[k]) for k in BIT_EQUAL)
    assert np.isfinite(d["img"]).all() and np.isfinite(d["img_rgb"]).all()


def test_the_device_draw_equals_its_host_twin(pre):
    """1024 seeds: integers and doubles bit-equal, rot_cs within 4 ulp of NumPy's; the device's own rot_cs fed to the host reproduces the device's batch
    bit for bit; the seed advances by the stride, and a second call draws anew."""
    from keypointfusion_amd import lib
    B = 1024
    seeds = (np.arange(B, dtype=np.int64) * 7919 + (1 << 40)) * np.where(np.arange(B) % 2, -1, 1)
    seed = _t(seeds)
    f64 = dict(device=_dev(), dtype=torch.float64)
    o = dict(mode=torch.zeros(B, device=_dev(), dtype=torch.int32), off=torch.zeros(B, 3, **f64), sc=torch.zeros(B, **f64), rot=torch.zeros(B, **f64),
             rot_cs=torch.zeros(B, 2, **f64), color=torch.zeros(B, 3, **f64))
    l = lib.load()
    call = lambda: lib.check(l.kpf_prep_aug_draw(seed.data_ptr(), B, 10.0, 0.2, 180.0, 0.2, 3, o["mode"].data_ptr(), o["off"].data_ptr(), o["sc"].data_ptr(),
                                                 o["rot"].data_ptr(), o["rot_cs"].data_ptr(), o["color"].data_ptr(), None), "kpf_prep_aug_draw")
    call()
    d = _cpu(o)
    h = P.draw_augment(seeds, 10.0, 0.2, 180.0, 0.2)
    for k in ("mode", "off", "sc", "rot", "color"):
        assert _same_bits(d[k], h[k]), k
    ulps = np.abs(d["rot_cs"] - h["rot_cs"]) / np.spacing(np.abs(h["rot_cs"]))
    print("rot_cs: max %.3g ulp from NumPy over %d seeds" % (ulps.max(), B))
    assert ulps.max() <= 4.0
    assert np.array_equal(seed.cpu().numpy(), seeds + 3)
    call()
    d2 = _cpu(o)
    assert not np.array_equal(d2["rot"], d["rot"]) and _same_bits(d2["rot"], P.draw_augment(seeds + 3)["rot"])


def test_drawn_batches_replay_with_fresh_draws_and_match_the_host(pre):
    """aug=None: draw, crop and sample.  The parameters returned, fed to the host function with the device's own rot_cs, reproduce the batch bit for bit;
    replaying the captured graph advances the seed and changes the draw."""
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor
    pre_g = DevicePreprocessor(cube=AC.CUBE, debug_candidates=True)
    names = ["right", "left", "corner", "left_edge", "fx_ne_fy", "wall", "right", "left"]
    items = [_inputs(n) for n in names]
    kw = _batch(items, [GC.draw(np.random.RandomState(0), 3)] * 8, range(500, 508))
    del kw["aug"]
    dev = _dev()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        pre_g.prepare_augmented(**kw, color_factor=0.2)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    assert kw["seed"].tolist() == list(range(508, 516))  # advanced by B
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pre_g.prepare_augmented(**kw, color_factor=0.2)
    draws = []
    for it in range(2):
        graph.replay()
        d = _cpu(out)
        a = {k: v.cpu().numpy() for k, v in out["aug"].items()}
        seeds = np.arange(508 + 8 * it, 516 + 8 * it)
        h = P.draw_augment(seeds, 10, 0.2, 180, 0.2)
        assert all(_same_bits(a[k], h[k]) for k in ("mode", "off", "sc", "rot", "color"))
        for b in range(8):
            aug = dict(mode=int(a["mode"][b]), off=a["off"][b], rot=float(a["rot"][b]), sc=float(a["sc"][b]), rot_cs=tuple(a["rot_cs"][b]), color=a["color"][b])
            _check_sample(d, b, GC.host_record(items[b], aug))
        draws.append(a["rot"].copy())
    assert not np.array_equal(draws[0], draws[1]) and kw["seed"].tolist() == list(range(524, 532))


def test_one_graphed_training_step_from_frames():
    """frames -> prepare_augmented -> train_batch -> GraphedTrainStep (B = 4, ConvNeXt-T, fp32, synthetic weights, frozen): the loss is finite, equals the
    eager iteration's on the same batch to the bits, and two seeds give different losses."""
    from conftest import synthetic_sd
    from keypointfusion_amd import training as T
    from keypointfusion_amd.model.model import KPFusion
    from keypointfusion_amd.parallel import live_parameters
    from keypointfusion_amd.preprocess_gpu import DevicePreprocessor, train_batch
    dev = _dev()
    net = "KPFusion-convnext-tiny"
    pre = DevicePreprocessor(cube=AC.CUBE)
    kw = _batch([_inputs(n) for n in ("right", "left", "corner", "fx_ne_fy")], [GC.draw(np.random.RandomState(0), 3)] * 4, [1, 2, 3, 4])
    del kw["aug"]

    class Loader:
        img_size, flip = 128, 1

    def loss_fn(mdl, bt):
        results, sws, _ = mdl(bt["img_rgb"], bt["img"], bt["pcl"], Loader(), bt["center"], bt["M"], bt["cube"], bt["cam_para"], 0.8)
        return T.kpfusion_loss(results, sws, bt["img"], bt["uvd_gt"], bt["xyz_gt"], epoch=0)[0]

    torch.manual_seed(0)
    m = KPFusion(net, "", 21, "dexycb", "")
    m.load_state_dict(synthetic_sd(net))
    m = m.to(dev).train()
    m.train_dropout = 0.0
    m.precision = "f32"
    live = live_parameters(m)
    opt = torch.optim.SGD(live, lr=0.0)
    batch = {k: v.clone() for k, v in train_batch(pre.prepare_augmented(**kw)).items()}
    assert set(batch) == {"img_rgb", "img", "pcl", "center", "M", "cube", "cam_para", "uvd_gt", "xyz_gt"} and batch["uvd_gt"].shape == (4, 21, 3)
    eager = float(loss_fn(m, batch))
    for p in m.parameters():
        p.grad = None
    step = T.GraphedTrainStep(m, opt, loss_fn, batch, warmup=1, params=live)
    first = float(step(batch))
    assert math.isfinite(first) and first == eager, (first, eager)
    kw["seed"].copy_(_t([1001, 1002, 1003, 1004], torch.int64))
    other = {k: v.clone() for k, v in train_batch(pre.prepare_augmented(**kw)).items()}
    second = float(step(other))
    assert math.isfinite(second) and second != first, (first, second)
