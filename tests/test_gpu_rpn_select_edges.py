"""``rpn_level_kernel`` / ``rpn_merge_kernel`` (csrc/proposals.hip) on the named cases of ``rpn_select_cases.py``, against
the independent reference ``rpn_select_ref.py`` (numpy, float64 boxes): selection with ties, levels smaller than
``pre_topk``, every top-k parameter at its edges, the scalar and the vector load path, decode edges and non-finite
deltas, suppression across the 64-candidate words of the greedy pass, IoU exactly on the threshold, the merge across
levels and an image without survivors.  ``demia_rpn_proposals`` is called through ``_lib`` directly: no engine, no
weights, no forward.

Every case runs on both selection paths (the 12-bit histogram select, and ``DEMIA_RPN_SELECT=radix``) and once more with
its images in reverse batch order.  Asserted per image: ``out_count``; the scores, bit for bit (they are input logits)
and in order; where every row came from ((level, h, w, a), recovered by matching the row against EVERY decoded anchor of
the image); the boxes; exact zeros from ``out_count`` on; finite outputs; an untouched guard behind each output.

The box bar is ``4 x F32_VS_REF x 2^-24 x S`` per coordinate, with ``S = |centre| + |d size| + exp(dsize) size`` of the
coordinate's axis (returned by the reference for every row) and ``rpn_select_cases.F32_VS_REF`` the measured distance of
a float32 decode from the float64 one over this table (``test_cpu_rpn_select_ref.py`` measures and guards it).  The kept
sets are compared exactly: the CPU test holds every case's decisions at least 1e-4 (IoU) and 1e-3 px away from their
thresholds, and the cases ON the NMS threshold have integer geometry, exact in float32.

What this table found: with the size deltas clamped by ``fminf`` (which returns the bound for a NaN) the four rows of
``decode_not_finite_deltas`` with a NaN width or height delta came out finite and were kept -- ``out_count`` 623 against
619 in image 0, on both selection paths.  The kernel's clamp now keeps a NaN, as ``torch.clamp`` does.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rpn_select_cases as T
import rpn_select_ref as REF

pytestmark = pytest.mark.gpu

BAR = 4.0 * T.F32_VS_REF * 2.0 ** -24
GUARD = 64                       # floats behind every output buffer that must keep their fill
FILL = 7.0


@pytest.fixture(scope="module")
def env(gpu_device):
    from deepemia_amd import _lib
    return dict(lib=_lib.load(), _lib=_lib, dev=gpu_device, cands={})


def _stream(env) -> int:
    return int(torch.cuda.current_stream(env["dev"]).cuda_stream)


def _upload(env, case, order):
    """The case's heads on the device, images in ``order``; ``base_offset`` floats off the allocation's alignment."""
    out = []
    for h in case.heads:
        a = np.ascontiguousarray(h[list(order)])
        buf = torch.zeros((a.size + 8,), dtype=torch.float32, device=env["dev"])
        view = buf[case.base_offset:case.base_offset + a.size]
        view.copy_(torch.from_numpy(a.reshape(-1)))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 * case.base_offset) % 16
        out.append((buf, view))
    return out


def _desc(env, case, heads, n, outs, ws, cell):
    _lib = env["_lib"]
    d = _lib.RpnDesc()
    for i, (_, view) in enumerate(heads):
        d.head[i] = int(view.data_ptr())
        d.H[i], d.W[i], d.stride[i] = case.heads[i].shape[1], case.heads[i].shape[2], int(case.strides[i])
    d.cell_anchors = cell.ctypes.data
    d.head_ld, d.N, d.img_h, d.img_w = case.head_ld, n, case.img_h, case.img_w
    d.pre_topk, d.post_topk, d.nms_thresh = case.pre_topk, case.post_topk, float(case.nms_thresh)
    d.out_boxes, d.out_scores, d.out_count, d.workspace = (_lib.ptr(t) for t in (*outs, ws))
    return d


def _outputs(env, n, post):
    dev = env["dev"]
    return (torch.full((n * post * 4 + GUARD,), FILL, dtype=torch.float32, device=dev),
            torch.full((n * post + GUARD,), FILL, dtype=torch.float32, device=dev),
            torch.full((n + GUARD,), -7, dtype=torch.int32, device=dev))


def run(env, case, order=None):
    """boxes [N, post, 4] f32, scores [N, post] f32, count [N] i32 (numpy) of one call; the guards are checked here."""
    n, post = case.n_images, case.post_topk
    order = range(n) if order is None else order
    heads = _upload(env, case, order)
    outs = _outputs(env, n, post)
    ws = torch.empty((int(env["lib"].demia_rpn_workspace_bytes(n)),), dtype=torch.uint8, device=env["dev"])
    cell = np.ascontiguousarray(case.cell, dtype=np.float32)
    d = _desc(env, case, heads, n, outs, ws, cell)
    env["_lib"].check(env["lib"].demia_rpn_proposals(C.byref(d), _stream(env)), f"demia_rpn_proposals({case.name})")
    torch.cuda.synchronize()
    b, s, c = (t.cpu().numpy() for t in outs)
    assert (b[n * post * 4:] == FILL).all() and (s[n * post:] == FILL).all() and (c[n:] == -7).all(), (case.name, "a guard behind an output was written")
    return b[:n * post * 4].reshape(n, post, 4), s[:n * post].reshape(n, post), c[:n]


def _candidates(env, case, n):
    key = (case.name, n)
    if key not in env["cands"]:
        cd = REF.all_candidates([h[n] for h in case.heads], case.cell, case.strides, case.img_h, case.img_w)
        bits = cd["score"].view(np.uint32)
        o = np.argsort(bits, kind="stable")
        env["cands"][key] = dict(src=cd["src"][o], box=cd["box"][o], bits=bits[o])
    return env["cands"][key]


def check_image(env, case, n, boxes, scores, count):
    """Problems of one image's output against the reference, as a list of strings, and the worst box error in bars."""
    r = T.reference(case)[n]
    k, post = r["count"], case.post_topk
    bad = []
    if int(count) != k:
        return [f"out_count {int(count)}, reference {k}"], 0.0
    if not (np.isfinite(boxes).all() and np.isfinite(scores).all()):
        bad.append("an output is not finite")
    if boxes[k:].any() or scores[k:].any() or np.signbit(boxes[k:]).any() or np.signbit(scores[k:]).any():
        bad.append("rows from out_count on are not exactly zero")
    if k == 0:
        return bad, 0.0
    gb, rb = scores[:k].view(np.uint32), r["scores"][:k].view(np.uint32)
    if not np.array_equal(gb, rb):
        i = int((gb != rb).argmax())
        return bad + [f"scores differ from row {i}: {scores[i]!r} against {r['scores'][i]!r}, which is (level, h, w, a) = {r['src'][i].tolist()}"], 0.0
    bar = BAR * np.stack([r["S"][:, 0], r["S"][:, 1]] * 2, axis=1)
    rel = np.abs(boxes[:k].astype(np.float64) - r["boxes"][:k]) / bar
    worst = float(rel.max())
    if worst > 1.0:
        i = int(rel.max(axis=1).argmax())
        bad.append(f"box of row {i} {boxes[i].tolist()} against {r['boxes'][i].tolist()}: {worst:.2f} of the bar; (level, h, w, a) = {r['src'][i].tolist()}")
    # where every row came from: among the anchors of the image with these score bits, the one whose decoded box is nearest
    cd = _candidates(env, case, n)
    lo, hi = np.searchsorted(cd["bits"], gb, "left"), np.searchsorted(cd["bits"], gb, "right")
    src = np.full((k, 4), -1, dtype=np.int64)
    one = hi - lo == 1
    src[one] = cd["src"][lo[one]]
    for i in np.nonzero(hi - lo > 1)[0]:
        dist = np.abs(cd["box"][lo[i]:hi[i]] - boxes[i].astype(np.float64)).max(axis=1)
        j = int(dist.argmin())
        # (anchors of equal score whose boxes coincide within the bar cannot be told apart by an output row: the reference's, if
        # it is one of them)
        twins = np.nonzero(dist <= dist[j] + bar[i].max())[0]
        mine = [t for t in twins if (cd["src"][lo[i] + t] == r["src"][i]).all()]
        src[i] = cd["src"][lo[i] + (mine[0] if mine else j)]
    if not np.array_equal(src, r["src"]):
        i = int((src != r["src"]).any(axis=1).argmax())
        bad.append(f"row {i} comes from (level, h, w, a) = {src[i].tolist()}, the reference's from {r['src'][i].tolist()}")
    return bad, worst


@pytest.mark.parametrize("select", ["two_pass", "radix"])
def test_case_table_against_the_reference(env, monkeypatch, select):
    if select == "radix":
        monkeypatch.setenv("DEMIA_RPN_SELECT", "radix")
    else:
        monkeypatch.delenv("DEMIA_RPN_SELECT", raising=False)
    failures, worst = [], (0.0, None)
    for case in T.CASES:
        boxes, scores, count = run(env, case)
        case_worst = 0.0
        for n in range(case.n_images):
            bad, w = check_image(env, case, n, boxes[n], scores[n], count[n])
            case_worst = max(case_worst, w)
            for b in bad:
                failures.append((case.name, f"image {n}", b, case.why))
                print(f"FAILED {select} {case.name} image {n}: {b}\n       ({case.why})")
        print(f"{select} {case.name:36s} counts {count.tolist()}  worst box {case_worst:.3f} of the bar")
        if case_worst > worst[0]:
            worst = (case_worst, (case.name, case.why))
    print(f"{select}: worst box error {worst[0]:.3f} of the bar (4 x {T.F32_VS_REF} x 2^-24 S) at {worst[1]}")
    assert not failures, (select, f"{len(failures)} failures (each printed above), the first:", failures[0], "worst box:", worst)


def test_reversed_batch_order_permutes_the_outputs_exactly(env, monkeypatch):
    """Per-image offsets into the heads, the workspace and the outputs: the images of every case in reverse order give the
    same rows, bit for bit, in reverse order."""
    monkeypatch.delenv("DEMIA_RPN_SELECT", raising=False)
    failures = []
    for case in T.CASES:
        a = run(env, case)
        b = run(env, case, order=range(case.n_images - 1, -1, -1))
        for what, x, y in zip(("boxes", "scores", "count"), a, b):
            if x.tobytes() != y[::-1].tobytes():
                failures.append((case.name, what, case.why))
    assert not failures, failures[:6]


def test_argument_guards_refuse_without_a_launch(env):
    """pre_topk 0 / 1001, post_topk 0 / 1025 and head_ld 14 are DEMIA_EINVAL and N = 0 is DEMIA_OK: pre-filled outputs keep
    their fill either way.  The valid call beside them writes every row."""
    case = T.BY_NAME["pre_topk_64"]
    n, post = case.n_images, case.post_topk
    heads = _upload(env, case, range(n))
    ws = torch.empty((int(env["lib"].demia_rpn_workspace_bytes(n)),), dtype=torch.uint8, device=env["dev"])
    cell = np.ascontiguousarray(case.cell, dtype=np.float32)
    einval, ok = -1, 0
    for field, value, want in (("pre_topk", 0, einval), ("pre_topk", 1001, einval), ("post_topk", 0, einval), ("post_topk", 1025, einval),
                               ("head_ld", 14, einval), ("N", 0, ok), (None, None, ok)):
        outs = _outputs(env, n, post)
        d = _desc(env, case, heads, n, outs, ws, cell)
        if field:
            setattr(d, field, value)
        status = env["lib"].demia_rpn_proposals(C.byref(d), _stream(env))
        torch.cuda.synchronize()
        assert status == want, (field, value, status, env["lib"].demia_last_error())
        b, s, c = (t.cpu().numpy() for t in outs)
        if field:
            assert (b == FILL).all() and (s == FILL).all() and (c == -7).all(), (field, value, "an output was written")
        else:
            assert not (b[:n * post * 4] == FILL).any() and not (s[:n * post] == FILL).any() and (c[:n] >= 0).all()
