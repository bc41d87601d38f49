"""A/B of `--task evaluate --visualize`: the scoring of ONE synthetic image (default 8192 x 8192 with roughly 900 final instances and
900 polygon annotations, boxes <= 120 px; `1024 300` for the small case) through both scorers of the evaluate task's pipeline mode,
`planes` and `crops`, with the error maps off and on -- REPS times each in one process, alternating (planes off, planes on, crops
off, crops on, planes off, ...), same inputs, same box.  Off is what the scorer did before the error maps existed.  No model runs:
the instances are synthetic blobs near the annotations, stored in both forms before the clock starts.

Per scorer and flag: `_score_pipeline_image` per image, the first repetition and the steady ones apart (host clock around work that
ends in a device synchronise), and the peak device memory of a repetition above what its input holds.  With the flag on the host's
PNG encode (Pillow's `Image.save`) is timed inside the call and reported apart, so `seconds - png_seconds` is the scoring with the
stage and its one copy.  The stage alone -- the two launches of `demia_mask_error_map` / `demia_crop_error_map` with the states'
upload -- is the device time between two events, median of five, next to its floor: one read and one write of the image, 6 H W
bytes at 6.3 TB/s.  The pictures of the two scorers are compared byte for byte.

    python scripts/gpu_error_map_ab.py [size=8192] [n=900] [reps=3] [out.json]
"""
import hashlib, json, statistics, sys, tempfile, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np, torch
from PIL import Image
from deepemia_amd import cocoeval as CE
from deepemia_amd.cropset import CropMaskSet
from deepemia_amd.functions.evaluate_model import _score_pipeline_image
from deepemia_amd.maskset import MaskOps

size = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
n = int(sys.argv[2]) if len(sys.argv) > 2 else 900
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_path = Path(sys.argv[4]).resolve() if len(sys.argv) > 4 else ROOT / "profiles" / f"error_map_ab_{size}.json"
HBM_BYTES_PER_SECOND = 6.3e12
ops = MaskOps("cuda:0")
rng = np.random.RandomState(8)
small = size < 4096
r_max, b_max = (30, 60) if small else (60, 120)

# annotations: concave rings
anns, centres = [], []
for i in range(n):
    cx, cy = rng.uniform(r_max + 10, size - r_max - 10, 2)
    k = rng.randint(4, 12)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    r = rng.uniform(8, r_max, k)
    pts = np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 2)
    anns.append({"segmentation": [[float(v) for v in pts]], "category_id": int(i % 2), "iscrowd": 0, "area": float(rng.uniform(100, 9000)),
                 "bbox": [float(cx - r_max), float(cy - r_max), float(cx + r_max), float(cy + r_max)], "bbox_mode": "XYXY_ABS"})
    centres.append((cx, cy))
rec = {"file_name": "synthetic.png", "image_id": 0, "height": size, "width": size, "annotations": anns}

# detections: one noisy blob near every annotation, of its class, packed on the host into rooms that are their tight boxes
rooms, words, areas = [], [], []
for cx, cy in centres:
    h, w = rng.randint(16, b_max), rng.randint(16, b_max)
    y0 = int(np.clip(cy - h // 2 + rng.randint(-10, 11), 0, size - h))
    x0 = int(np.clip(cx - w // 2 + rng.randint(-10, 11), 0, size - w))
    sub = rng.rand(h, w) < .85
    sub[0, :] = sub[-1, :] = sub[:, 0] = sub[:, -1] = True            # (the window is the tight box)
    c0, wc = x0 >> 5, ((x0 + w - 1) >> 5) - (x0 >> 5) + 1
    bits = np.zeros((h, wc * 32), dtype=bool)
    bits[:, x0 - 32 * c0: x0 - 32 * c0 + w] = sub
    words.append(np.packbits(bits.reshape(h, wc, 32), axis=-1, bitorder="little").view(np.uint32).reshape(-1))
    rooms.append((y0, x0, y0 + h - 1, x0 + w - 1))
    areas.append(int(sub.sum()))
room_h = np.asarray(rooms, dtype=np.int32)
area_h = np.asarray(areas, dtype=np.int32)
tab = ops.upload(np.concatenate([room_h.reshape(-1), area_h, np.concatenate(words).view(np.int32)]))
cset = CropMaskSet(ops, (size, size), room_h, tab[5 * n:], tab[:4 * n].view(n, 4), tab[4 * n:5 * n])
planes = cset.to_planes()
tabs = (area_h.astype(np.int64), room_h)
scores = [float(v) for v in rng.uniform(.3, 1, n)]
classes = [int(i % 2) for i in range(n)]
image = torch.from_numpy(rng.randint(0, 256, (size, size, 3)).astype(np.uint8)).to(ops.device)
forms = {"planes": planes, "crops": cset}
input_bytes = {"planes": planes.numel() * 4, "crops": cset.words * 4 + n * 36}
ids = {0: 0, 1: 1}
IOU, ALPHA = 0.2, 96                                                  # (the random boxes rarely reach 0.5 against their polygons)
line = CE.error_map_line(size, size)

png = [0.0]
save = Image.Image.save
def timed_save(self, *a, **k):
    t0 = time.perf_counter()
    try:
        return save(self, *a, **k)
    finally:
        png[0] += time.perf_counter() - t0
Image.Image.save = timed_save
states = {}
make_states = CE.error_map_states
def kept_states(*a):
    states["d"], states["g"] = make_states(*a)
    return states["d"], states["g"]
CE.error_map_states = kept_states

tmp = Path(tempfile.mkdtemp(prefix="error_map_ab_"))
runs_by = {(f, flag): [] for f in forms for flag in (False, True)}
digest, picture = {}, {}
for rep in range(reps):
    for form, packed in forms.items():
        for flag in (False, True):                       # alternating: planes off, planes on, crops off, crops on, ...
            tables = {"bbox": CE.EvalTables(), "segm": CE.EvalTables()}
            maps = CE.ErrorMaps(str(tmp / form), IOU, ALPHA, None) if flag else None
            png[0] = 0.0
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            rows = _score_pipeline_image(ops, rec, (size, size), packed, scores, classes, tabs, tables, ids, maps=maps, image=image if flag else None)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            peak = int(torch.cuda.max_memory_allocated()) - before
            h = hashlib.sha256((repr(rows) + repr([tables[t].cat(k).tolist() for t in tables for k in ("iou", "d_area", "g_area")])).encode()).hexdigest()
            digest.setdefault(form, h)
            assert digest[form] == h, "a repetition, or the flag, gave other rows"
            if flag:
                p = hashlib.sha256(np.asarray(Image.open(maps.image_path(0, "synthetic.png")).convert("RGB")).tobytes()).hexdigest()
                picture.setdefault(form, (p, maps.rows[0][2:12]))
                assert picture[form] == (p, maps.rows[0][2:12]), "a repetition painted another picture"
            runs_by[form, flag].append(dict(seconds=dt, png_seconds=png[0], peak_bytes_above_input=peak))
            print(f"rep {rep} {form:6s} {'on ' if flag else 'off'}: {dt:.3f} s (PNG encode {png[0]:.3f} s), peak {peak / 2**20:.1f} MiB above its input "
                  f"({input_bytes[form] / 2**20:.1f} MiB)", flush=True)

# the stage alone: device time between two events, median of five (one warm launch first)
polys = [a["segmentation"] for a in anns]
g_planes, _, g_bbox = CE.rasterize_polygons(ops, polys, size, size)
g_set, _ = CE.rasterize_polygons_crop(ops, polys, size, size)
d_bbox = ops.upload(room_h)
stage = {"planes": lambda: ops.error_map(planes, d_bbox, states["d"], g_planes, g_bbox, states["g"], image, ALPHA, line, W=size),
         "crops": lambda: cset.error_map(g_set, states["d"], states["g"], image, ALPHA, line, bbox=d_bbox)}
stage_ms = {}
for form, run in stage.items():
    run()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    stage_ms[form] = ms

floor_ms = 1e3 * 6 * size * size / HBM_BYTES_PER_SECOND
res = {"image": f"{size}x{size}", "instances": n, "annotations": len(anns), "box_edge_max_px": b_max, "reps_per_case": reps,
       "order": "alternating planes off, planes on, crops off, crops on", "iou": IOU, "alpha": ALPHA, "line": line,
       "matched_pairs": picture["planes"][1][2], "counts_agree_excess_missing_ignored": picture["planes"][1][6:10],
       "same_rows_off_and_on_and_in_both_scorers": len(set(digest.values())) == 1, "row_digest": digest,
       "same_picture_in_both_scorers": picture["planes"] == picture["crops"], "picture_digest": {f: v[0] for f, v in picture.items()},
       "stage_floor_ms_6HW_bytes_at_6.3_TB_per_s": floor_ms, "device": torch.cuda.get_device_name(0), "scorers": {}}
for form in forms:
    entry = {"input_bytes": int(input_bytes[form]), "stage_alone_device_ms": stage_ms[form], "stage_alone_device_ms_median": statistics.median(stage_ms[form])}
    for flag in (False, True):
        rr = runs_by[form, flag]
        steady = [r["seconds"] for r in rr[1:]]
        entry["on" if flag else "off"] = dict(first_image_seconds=rr[0]["seconds"], steady_seconds=steady,
                                              steady_median_seconds=statistics.median(steady) if steady else None,
                                              png_encode_seconds=[r["png_seconds"] for r in rr] if flag else None,
                                              peak_bytes_above_input=max(r["peak_bytes_above_input"] for r in rr))
    res["scorers"][form] = entry
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res))
