"""``box_detections_kernel<WIDE>`` (csrc/proposals.hip) on the named cases of ``box_dets_cases.py``, against the
independent reference ``box_dets_ref.py`` (numpy, float64 scores and boxes): ``prop_count`` from 0 to past ``R`` with
garbage behind it, exact and padded ``ld``, one to eight classes, softmax extremes and non-finite logits, scores ON the
threshold, the size clamp, non-finite boxes in classes nobody asks for, boxes clipped to zero area, ties across
proposals, classes, chunk edges and the ``topk`` cut, chains and clusters within and across 64-candidate chunks, IoU
exactly on the threshold, 1000 | 1001 candidates, all 4096 sort slots, and every ``topk`` edge.  ``demia_box_detections``
is called through ``_lib`` directly: no engine, no weights, no forward.

Asserted per image: ``det_count``; the classes, exactly and in order; scores and boxes within the bars; exact zeros from
``det_count`` on; finite outputs; an untouched guard behind each of the four outputs.  The bars are ``4 x
F32_VS_REF_SCORE x 2^-24`` for a score and ``4 x F32_VS_REF_BOX x 2^-24 x S`` for a coordinate, with ``S = |centre| +
|d size| + exp(dsize) size`` of the coordinate's axis (returned by the reference for every row) and the two records of
``box_dets_cases.py`` the measured distance of a float32 restatement from the float64 reference over this table
(``test_cpu_box_dets_ref.py`` measures and guards them).  The kept sets and their order are compared exactly: the CPU test
holds every decision of the table away from its threshold, and the cases ON a threshold are exact in float32.

Every case runs once more with its images in reverse batch order, image by image in batches of one, and at ``topk`` =
100, 128, 129 and 1000 (prefixes of one another across the one-wave | sixteen-wave switch), all bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import box_dets_cases as T

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
SCORE_BAR = 4.0 * T.F32_VS_REF_SCORE * ULP
BOX_BAR = 4.0 * T.F32_VS_REF_BOX * ULP
GUARD = 64                       # elements behind every output buffer that must keep their fill
FILL, IFILL = 7.0, -7
EINVAL, OK = -1, 0


@pytest.fixture(scope="module")
def env(gpu_device):
    from deepemia_amd import _lib
    return dict(lib=_lib.load(), _lib=_lib, dev=gpu_device, runs={})


def _stream(env) -> int:
    return int(torch.cuda.current_stream(env["dev"]).cuda_stream)


def _outputs(env, n, topk):
    dev = env["dev"]
    return (torch.full((n * topk * 4 + GUARD,), FILL, dtype=torch.float32, device=dev),
            torch.full((n * topk + GUARD,), FILL, dtype=torch.float32, device=dev),
            torch.full((n * topk + GUARD,), IFILL, dtype=torch.int32, device=dev),
            torch.full((n + GUARD,), IFILL, dtype=torch.int32, device=dev))


def _desc(env, ins, outs, n, r, ld, k, img_h, img_w, score_thresh, nms_thresh, topk):
    _lib = env["_lib"]
    return _lib.DetsDesc(_lib.ptr(ins[0]), ld, _lib.ptr(ins[1]), _lib.ptr(ins[2]), n, r, k, img_h, img_w, float(score_thresh), float(nms_thresh),
                         topk, *(_lib.ptr(t) for t in outs))


def _fetch(outs, n, topk, what):
    b, s, c, m = (t.cpu().numpy() for t in outs)
    assert (b[n * topk * 4:] == FILL).all() and (s[n * topk:] == FILL).all() and (c[n * topk:] == IFILL).all() and (m[n:] == IFILL).all(), \
        (what, "a guard behind an output was written")
    return b[:n * topk * 4].reshape(n, topk, 4), s[:n * topk].reshape(n, topk), c[:n * topk].reshape(n, topk), m[:n]


def run(env, case, order=None, topk=None):
    """boxes [N, topk, 4] f32, scores [N, topk] f32, classes [N, topk] i32, count [N] i32 (numpy) of one call on the images
    ``order`` of the case; exact-size inputs, the guards behind the outputs are checked here."""
    order = tuple(range(case.n_images) if order is None else order)
    topk = case.topk if topk is None else topk
    key = (case.name, order, topk)
    if key not in env["runs"]:
        dev, n = env["dev"], len(order)
        ins = (torch.from_numpy(np.ascontiguousarray(case.logits[list(order)])).to(dev), torch.from_numpy(np.ascontiguousarray(case.props[list(order)])).to(dev),
               torch.from_numpy(np.ascontiguousarray(case.prop_count[list(order)])).to(dev))
        assert ins[1].data_ptr() % 16 == 0
        outs = _outputs(env, n, topk)
        d = _desc(env, ins, outs, n, case.R, case.ld, case.K, case.img_h, case.img_w, case.score_thresh, case.nms_thresh, topk)
        env["_lib"].check(env["lib"].demia_box_detections(C.byref(d), _stream(env)), f"demia_box_detections({case.name})")
        torch.cuda.synchronize()
        res = _fetch(outs, n, topk, case.name)
        for a in res:
            a.setflags(write=False)
        env["runs"][key] = res
    return env["runs"][key]


def check_image(case, n, boxes, scores, classes, count):
    """Problems of one image's output against the reference, as a list of strings, and the worst score and box error in bars."""
    r = T.reference(case)[n]
    k = r["count"]
    if int(count) != k:
        return [f"det_count {int(count)}, reference {k} (candidates {r['ncand']}, survivors {r['survivors']})"], 0.0, 0.0
    bad = []
    if not (np.isfinite(boxes).all() and np.isfinite(scores).all()):
        bad.append("an output is not finite")
    if boxes[k:].any() or scores[k:].any() or classes[k:].any() or np.signbit(boxes[k:]).any() or np.signbit(scores[k:]).any():
        bad.append("rows from det_count on are not exactly zero")
    if k == 0:
        return bad, 0.0, 0.0
    if not np.array_equal(classes[:k], r["classes"][:k]):
        i = int((classes[:k] != r["classes"][:k]).argmax())
        return bad + [f"classes differ from row {i}: {int(classes[i])} against {int(r['classes'][i])}, which is (row, class) = {r['src'][i].tolist()}"], 0.0, 0.0
    es = np.abs(scores[:k].astype(np.float64) - r["scores"][:k]) / SCORE_BAR
    if es.max() > 1.0:
        i = int(es.argmax())
        bad.append(f"score of row {i} {scores[i]!r} against {r['scores'][i]!r}: {es.max():.2f} of the bar; (row, class) = {r['src'][i].tolist()}")
    bar = BOX_BAR * np.stack([r["S"][:, 0], r["S"][:, 1]] * 2, axis=1)
    eb = np.abs(boxes[:k].astype(np.float64) - r["boxes"][:k]) / bar
    if eb.max() > 1.0:
        i = int(eb.max(axis=1).argmax())
        bad.append(f"box of row {i} {boxes[i].tolist()} against {r['boxes'][i].tolist()}: {eb.max():.2f} of the bar; (row, class) = {r['src'][i].tolist()}")
    return bad, float(es.max()), float(eb.max())


def test_case_table_against_the_reference(env):
    failures, worst_s, worst_b = [], (0.0, None), (0.0, None)
    for case in T.CASES:
        boxes, scores, classes, count = run(env, case)
        ws = wb = 0.0
        for n in range(case.n_images):
            bad, s, b = check_image(case, n, boxes[n], scores[n], classes[n], count[n])
            ws, wb = max(ws, s), max(wb, b)
            for x in bad:
                failures.append((case.name, f"image {n}", x, case.why))
                print(f"FAILED {case.name} image {n}: {x}\n       ({case.why})")
        print(f"{case.name:42s} counts {count.tolist()}  worst score {ws:.3f}, worst box {wb:.3f} of the bar")
        if ws > worst_s[0]:
            worst_s = (ws, case.name)
        if wb > worst_b[0]:
            worst_b = (wb, case.name)
    print(f"worst score error {worst_s[0]:.3f} of the bar (4 x {T.F32_VS_REF_SCORE} x 2^-24) at {worst_s[1]}; "
          f"worst box error {worst_b[0]:.3f} of the bar (4 x {T.F32_VS_REF_BOX} x 2^-24 S) at {worst_b[1]}")
    assert not failures, (f"{len(failures)} failures (each printed above), the first:", failures[0])


def test_reversed_batch_order_permutes_the_outputs_exactly(env):
    """Per-image offsets into the logits (n R ld), the proposals and counts (n R, n) and the outputs (n topk): the images of
    every case in reverse order give the same rows, bit for bit, in reverse order."""
    failures = []
    for case in T.CASES:
        a = run(env, case)
        b = run(env, case, order=range(case.n_images - 1, -1, -1))
        for what, x, y in zip(("boxes", "scores", "classes", "count"), a, b):
            if x.tobytes() != y[::-1].tobytes():
                failures.append((case.name, what, case.why))
    assert not failures, failures[:6]


def test_an_image_alone_equals_the_image_in_its_batch(env):
    """Each image in a batch of one gives the rows it gets inside its batch, bit for bit."""
    failures = []
    for case in T.CASES:
        a = run(env, case)
        for n in range(case.n_images):
            b = run(env, case, order=(n,))
            for what, x, y in zip(("boxes", "scores", "classes", "count"), a, b):
                if x[n].tobytes() != y[0].tobytes():
                    failures.append((case.name, n, what, case.why))
    assert not failures, failures[:6]


def test_topk_prefixes_across_the_wave_switch(env):
    """Every case at topk = 100, 128 (one wave scans the kept list), 129 and 1000 (sixteen waves share it): the shorter list
    is the first rows of the longer one, bit for bit, and det_count = min(topk, det_count at 1000)."""
    failures = []
    for case in T.CASES:
        fb, fs, fc, fn = run(env, case, topk=1000)
        for topk in (100, 128, 129):
            b, s, c, m = run(env, case, topk=topk)
            if not (b.tobytes() == fb[:, :topk].tobytes() and s.tobytes() == fs[:, :topk].tobytes() and c.tobytes() == fc[:, :topk].tobytes()):
                failures.append((case.name, topk, "rows", case.why))
            if m.tolist() != np.minimum(fn, topk).tolist():
                failures.append((case.name, topk, "det_count", m.tolist(), fn.tolist()))
    assert not failures, failures[:6]


def test_argument_guards_refuse_without_a_launch(env):
    """K = 0, score_thresh = 0, topk 0 and 1025, ld = 5 K and R x min(K, floor(1 / thresh)) = 4097 are DEMIA_EINVAL, N = 0 is
    DEMIA_OK: pre-filled outputs keep their fill either way.  The valid call beside them (4096 candidates' worth of rows)
    writes every row."""
    dev = env["dev"]
    n, r, k, ld, topk, cap = 2, 4096, 1, 6, 100, 1025
    rng = np.random.default_rng(7)
    logits = np.zeros((n, r + 1, ld), dtype=np.float32)                       # room for R = 4097
    logits[..., 0] = rng.uniform(1.0, 3.0, (n, r + 1)).astype(np.float32)     # every row a candidate at thresh 0.5
    ins = (torch.from_numpy(logits).to(dev), torch.from_numpy(T.grid_props(n, r + 1, cols=64)).to(dev),
           torch.full((n,), r, dtype=torch.int32, device=dev))
    for field, value, want in (("K", 0, EINVAL), ("score_thresh", 0.0, EINVAL), ("topk", 0, EINVAL), ("topk", 1025, EINVAL), ("ld", 5 * k, EINVAL),
                               ("R", r + 1, EINVAL), ("N", 0, OK), (None, None, OK)):
        outs = _outputs(env, n, cap)                                           # room for topk = 1025
        d = _desc(env, ins, outs, n, r, ld, k, 800, 800, 0.5, 0.5, topk)
        if field:
            setattr(d, field, value)
        status = env["lib"].demia_box_detections(C.byref(d), _stream(env))
        torch.cuda.synchronize()
        assert status == want, (field, value, status, env["lib"].demia_last_error())
        b, s, c, m = (t.cpu().numpy() for t in outs)
        if field:
            assert (b == FILL).all() and (s == FILL).all() and (c == IFILL).all() and (m == IFILL).all(), (field, value, "an output was written")
        else:
            assert m[:n].tolist() == [topk, topk] and (m[n:] == IFILL).all()
            assert not (b[:n * topk * 4] == FILL).any() and not (s[:n * topk] == FILL).any() and not (c[:n * topk] == IFILL).any()
            assert (b[n * topk * 4:] == FILL).all() and (s[n * topk:] == FILL).all() and (c[n * topk:] == IFILL).all()
