"""``roi_align_kernel`` / ``roi_order_kernel`` (csrc/roialign.hip) at edge geometry, against an independent f64 reference.

The boxes are the named table of ``roi_align_cases.py`` (level boundaries, the boundary between the separable "tables"
path and the per-sample fallback, samples exactly on -1 and on ``size``, bins and boxes outside the map, zero-area boxes,
bins of 7 samples that touch NINE pixels, 60 random boxes) on a small two-image pyramid; the reference is
``roi_align_ref.py`` (direct per-sample form, f32 geometry in torchvision's order, f64 weights and sums).  Every failure
names the worst case of the table.

Tolerances, all relative to ``amax`` = the largest |feature| of the box's level in its image:
  * the reference against the CPU oracle (torch f32, another summation order), same table, 256 channels, P in 1, 2, 7,
    14, 15: largest |oracle - reference| / amax = 1.319e-7 (``roi_align_cases.ORACLE_VS_REF``, measured and guarded by
    ``test_cpu_roi_align_ref.py``);
  * exact-f32 kernel: 4 x that figure = 5.28e-7 (a third summation order; a wrong tap weight shows at 1e-2 or more);
  * P32 planes: the f32 bound plus the storage floor, measured per image on the reference's own output as the largest
    |to_f32(from_f32(ref)) - ref| at the scale the kernel must choose (the coarsest of the four levels);
  * bf16: the f32 bound plus 2^-8 |ref| per element (one step of the output type).
Rows beyond ``count`` are exactly zero; integer work (the launch order) is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import roi_align_cases as T
import roi_align_ref as REF

pytestmark = pytest.mark.gpu

F32_TOL = 4.0 * T.ORACLE_VS_REF
LEVELS = ("p2", "p3", "p4", "p5")


@pytest.fixture(scope="module")
def env(gpu_device):
    from deepemia_amd import synth
    from deepemia_amd.engine import MaskRCNNEngine

    sd = synth.random_d2_state_dict(50, 2, seed=0)
    eng = MaskRCNNEngine(sd, 50, 2, 0.3, gpu_device, "f32")            # the engines only lend their roi_align: no forward is run
    eng2 = MaskRCNNEngine(sd, 50, 2, 0.3, gpu_device, "f16x2")
    feats = T.features()
    return dict(sd=sd, eng=eng, eng2=eng2, dev=gpu_device, feats=feats,
                feats_dev={k: torch.from_numpy(f).to(gpu_device) for k, f in zip(LEVELS, feats)},
                boxes=torch.from_numpy(np.stack([T.BOXES] * T.N_IMAGES)).contiguous().to(gpu_device), refs={})


def reference(env, key, feats, P):
    """[N, R, P, P, C] f64 and the level of every box, computed once per (features, P) and shared (read only)."""
    k = (key, P)
    if k not in env["refs"]:
        out, dg = REF.roi_pool([np.moveaxis(f, 0, 2) for f in feats], T.BOXES, P)         # [R, P, P, N, C]
        out = np.ascontiguousarray(np.moveaxis(out, 3, 0))
        out.setflags(write=False)
        env["refs"][k] = (out, np.array([d["level"] for d in dg]))
    return env["refs"][k]


def level_amax(feats):
    return np.stack([np.abs(f).reshape(f.shape[0], -1).max(axis=1) for f in feats]).astype(np.float64)     # [level, image]


def check(got, ref, lv, amax, count, tol, what, extra=None):
    """``got``, ``ref``: [N, R, P, P, C]; rows r >= count[n] exactly zero, the others within tol * amax[level, n] (+ extra)."""
    worst = (-1.0, None)
    assert np.isfinite(got).all(), what
    for n in range(got.shape[0]):
        c = int(count[n])
        assert not got[n, c:].any(), (what, "rows beyond count are not zero", n, [T.NAMES[i] for i in range(c, got.shape[1]) if got[n, i].any()][:5])
        if c == 0:
            continue
        diff = np.abs(got[n, :c].astype(np.float64) - ref[n, :c])
        if extra is not None:
            diff = np.maximum(diff - extra[n][:c], 0.0)
        err = diff.reshape(c, -1).max(axis=1) / amax[lv[:c], n]
        i = int(err.argmax())
        print(f"{what}: image {n}, {c} rows, worst {err[i]:.3e} of amax (bound {tol:.3e}) at {T.NAMES[i]}")
        if err[i] > worst[0]:
            worst = (float(err[i]), (T.NAMES[i], n, T.CASES[i].why))
    assert worst[0] <= tol, (what, worst, tol)


@pytest.mark.parametrize("P", T.POOL_SIZES)
def test_f32_kernel_on_the_case_table(env, P):
    eng, dev = env["eng"], env["dev"]
    ref, lv = reference(env, "f32", env["feats"], P)
    amax = level_amax(env["feats"])
    for count in ([T.R, T.R - 9], [0, 3]):
        cnt = torch.tensor(count, dtype=torch.int32, device=dev)
        got = eng.roi_align(env["feats_dev"], env["boxes"], cnt, P).cpu().numpy()
        assert got.shape == (T.N_IMAGES, T.R, P, P, T.C)
        check(got, ref, lv, amax, count, F32_TOL, f"f32 P={P} count={count}")
        if count[0] == T.R:
            # the boxes that pool to nothing (zero area, wholly outside): exactly zero, in the reference as well
            for i, c in enumerate(T.CASES):
                if c.expect.get("zero"):
                    assert not ref[:, i].any() and not got[:, i].any(), c.name


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("P", [7, 14])
def test_p32_kernel_on_the_case_table(env, P, groups):
    from deepemia_amd import p32

    eng2, dev = env["eng2"], env["dev"]
    planes = {k: p32.from_f32(env["feats_dev"][k], groups=groups) for k in LEVELS}
    deq = [p32.to_f32(planes[k]).cpu().numpy() for k in LEVELS]                 # what the kernel reads, as f32
    ref, lv = reference(env, f"p32g{groups}", deq, P)
    amax = level_amax(deq)
    count = [T.R, T.R - 9]
    cnt = torch.tensor(count, dtype=torch.int32, device=dev)
    out = eng2.roi_align(planes, env["boxes"], cnt, P)
    assert out.groups == groups and out.shape == (T.N_IMAGES, T.R, P, P, T.C)
    # the output's meta: the largest amax and the coarsest (smallest) scale of the four levels, per scale group
    meta = torch.stack([planes[k].meta for k in LEVELS]).cpu().numpy()          # [level, groups, 2]
    want_meta = np.stack([meta[:, :, 0].max(axis=0), meta[:, :, 1].min(axis=0)], axis=1)
    np.testing.assert_array_equal(out.meta.cpu().numpy(), want_meta)
    # storage floor: the reference's own output through the planes at that scale, per image
    floor = []
    for n in range(T.N_IMAGES):
        r32 = torch.from_numpy(ref[n].astype(np.float32))
        q = p32.to_f32(p32.from_f32(r32, bound=float(want_meta[n if groups > 1 else 0, 0]))).numpy().astype(np.float64)
        floor.append(float(np.abs(q - ref[n]).max()))
        print(f"p32 P={P} groups={groups}: storage floor of image {n}: {floor[-1]:.3e} = {floor[-1] / amax[:, n].min():.3e} of the smallest level amax")
    got = p32.to_f32(out).cpu().numpy()
    check(got, ref, lv, amax, count, F32_TOL, f"p32 P={P} groups={groups}", extra=[np.full((T.R, 1, 1, 1), f) for f in floor])


def test_bf16_kernel_on_the_case_table(env):
    from conftest import needs_dev_build
    needs_dev_build("bf16")
    from deepemia_amd.engine import MaskRCNNEngine

    dev = env["dev"]
    eng = MaskRCNNEngine(env["sd"], 50, 2, 0.3, dev, "bf16")
    fb = {k: env["feats_dev"][k].to(torch.bfloat16) for k in LEVELS}
    rounded = [fb[k].float().cpu().numpy() for k in LEVELS]
    amax = level_amax(rounded)
    count = [T.R, T.R - 9]
    cnt = torch.tensor(count, dtype=torch.int32, device=dev)
    for P in (7, 14):
        ref, lv = reference(env, "bf16", rounded, P)
        got = eng.roi_align(fb, env["boxes"], cnt, P).float().cpu().numpy()
        check(got, ref, lv, amax, count, F32_TOL, f"bf16 P={P}", extra=[np.abs(ref[n]) * 2.0 ** -8 for n in range(T.N_IMAGES)])


@pytest.mark.parametrize("channels", [64, 4])
def test_direct_descriptor_with_fewer_channels_switches_lanes_off(env, channels):
    """The library takes any C % 4 == 0 up to 256 (lanes with 4 lane >= C do nothing): C = 64 and C = 4 in f32, P = 7, on the
    named cases (the table without its random boxes); a zeroed guard behind ``out`` stays untouched and every row of
    ``out`` is written."""
    from deepemia_amd import _lib

    eng, dev = env["eng"], env["dev"]
    P = 7
    rows = [i for i, c in enumerate(T.CASES) if not c.name.startswith("bulk_")]
    r = len(rows)
    ref_all, lv_all = reference(env, "f32", env["feats"], P)
    ref, lv = ref_all[:, rows][..., :channels], lv_all[rows]
    feats = [env["feats_dev"][k][..., :channels].contiguous() for k in LEVELS]
    boxes = env["boxes"][:, rows].contiguous()
    count = [r, r - 5]
    cnt = torch.tensor(count, dtype=torch.int32, device=dev)
    n_out, guard = T.N_IMAGES * r * P * P * channels, 4096
    buf = torch.zeros(n_out + guard, dtype=torch.float32, device=dev)
    buf[:n_out] = 7.0                                                       # (no pooled value is exactly 7)
    d = _lib.RoiAlignDesc()
    for i, f in enumerate(feats):
        d.feat[i] = _lib.ptr(f)
        d.H[i], d.W[i] = f.shape[1], f.shape[2]
    d.N, d.R, d.C, d.P, d.dtype = T.N_IMAGES, r, channels, P, _lib.F32
    d.boxes, d.count, d.out = _lib.ptr(boxes), _lib.ptr(cnt), _lib.ptr(buf)
    _lib.check(eng.lib.demia_roi_align(C.byref(d), eng._stream()), "demia_roi_align")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert not host[n_out:].any(), "the guard behind out was written"
    got = host[:n_out].reshape(T.N_IMAGES, r, P, P, channels)
    assert not (got == 7.0).any(), "an element of out was not written"
    assert np.isfinite(got).all()
    names = [T.NAMES[i] for i in rows]
    amax = level_amax([f[..., :channels] for f in env["feats"]])
    worst = (-1.0, None)
    for n in range(T.N_IMAGES):
        c = count[n]
        assert not got[n, c:].any()
        err = np.abs(got[n, :c].astype(np.float64) - ref[n, :c]).reshape(c, -1).max(axis=1) / amax[lv[:c], n]
        i = int(err.argmax())
        print(f"C={channels}: image {n}, worst {err[i]:.3e} of amax (bound {F32_TOL:.3e}) at {names[i]}")
        worst = max(worst, (float(err[i]), names[i]))
    assert worst[0] <= F32_TOL, worst


def order_keys(boxes: np.ndarray):
    """The documented sort key of a pooled row: (level, cy >> 3, cx, index) with the box centre in level pixels, f32."""
    f32 = np.float32
    keys = []
    for t, b in enumerate(boxes):
        lv = REF.assign_level(b)
        scale = f32(1.0) / f32(REF.STRIDES[lv])
        cy = min(max(int((b[1] + b[3]) * f32(0.5) * scale), 0), 4095)
        cx = min(max(int((b[0] + b[2]) * f32(0.5) * scale), 0), 4095)
        keys.append((lv, cy >> 3, cx, t))
    return keys


@pytest.mark.parametrize("r", [8, 100, 1024])
def test_launch_order_on_the_case_table(env, r):
    """``demia_roi_order``: a permutation of each image's rows, pooled rows (index < count) before unused ones and sorted by the
    documented key, dealt to the XCDs in runs of R / 8 when 8 divides R; ``count`` = R, 1 and 0; the pooled output is bit-equal
    to the unordered launch."""
    from deepemia_amd import _lib

    eng, dev = env["eng"], env["dev"]
    tab = np.resize(T.BOXES, (r, 4)) if r > T.R else T.BOXES[:r]
    boxes = torch.from_numpy(np.stack([tab] * T.N_IMAGES)).contiguous().to(dev)
    keys = order_keys(tab)
    sure = [REF.level_is_unambiguous(b) for b in tab]
    P = 7 if r > 100 else 14
    for count in ([r, 1], [0, r]):
        cnt = torch.tensor(count, dtype=torch.int32, device=dev)
        order = torch.empty((T.N_IMAGES * r,), dtype=torch.int32, device=dev)
        _lib.check(eng.lib.demia_roi_order(_lib.ptr(boxes), _lib.ptr(cnt), T.N_IMAGES, r, _lib.ptr(order), eng._stream()), "demia_roi_order")
        o = order.cpu().numpy().reshape(T.N_IMAGES, r)
        for n in range(T.N_IMAGES):
            assert sorted(o[n].tolist()) == list(range(n * r, (n + 1) * r)), (r, count, n)
            per = r // 8
            ranked = [int(o[n][(s % per) * 8 + s // per] if r % 8 == 0 else o[n][s]) - n * r for s in range(r)]     # sorted rank -> row
            c = count[n]
            assert sorted(ranked[:c]) == list(range(c)), ("pooled rows first", r, count, n)
            assert ranked[c:] == list(range(c, r)), ("unused rows in index order", r, count, n)
            want = [t for (_, _, _, t) in sorted(keys[:c]) if sure[t]]
            assert [t for t in ranked[:c] if sure[t]] == want, (r, count, n)
        old = eng.roi_order
        try:
            eng.roi_order = True
            a = eng.roi_align(env["feats_dev"], boxes, cnt, P).clone()
            eng.roi_order = False
            b = eng.roi_align(env["feats_dev"], boxes, cnt, P)
        finally:
            eng.roi_order = old
        assert torch.equal(a, b), (r, count)
