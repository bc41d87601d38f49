"""A/B of `evaluation.score_frame`: the scoring of ONE synthetic 8192 x 8192 image with roughly 900 final instances and 900
polygon annotations (boxes <= 120 px) through both scorers of the evaluate task's
pipeline mode -- `planes` (detections as full-frame planes, every annotation rasterised into one) and `crops` (the same
detections as a CropMaskSet, the ground truth built as one too) -- REPS times each in one process, alternating (planes, crops,
planes, ...), same inputs, same box.  No model runs: the instances are synthetic blobs near the annotations, stored in both
forms before the clock starts, so the figures are the scoring alone (`_score_pipeline_image`: ground truth, cross matrix, run
lengths, the one device-to-host copy, strings and table rows).

Per scorer: the first repetition and the steady ones apart (host clock around work that ends in a device synchronise), the peak
device memory of a repetition above what its input holds (`torch.cuda.max_memory_allocated` after `reset_peak_memory_stats`,
minus the bytes allocated before the call), the bytes of the input form itself, whether both scorers gave the same rows, and the
digest of each scorer's rows and tables (`row_digest`: equal digests at two commits mean the scoring computed the same).

    python scripts/gpu_eval_frame_ab.py [size=8192] [n=900] [reps=4] [out.json]
"""
import hashlib, json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np, torch
from deepemia_amd import cocoeval as CE
from deepemia_amd.cropset import CropMaskSet
from deepemia_amd.functions.evaluate_model import _score_pipeline_image
from deepemia_amd.maskset import MaskOps

size = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
n = int(sys.argv[2]) if len(sys.argv) > 2 else 900
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
out_path = Path(sys.argv[4]).resolve() if len(sys.argv) > 4 else ROOT / "profiles" / f"eval_frame_ab_{size}.json"
ops = MaskOps("cuda:0")
rng = np.random.RandomState(8)

# annotations: concave rings with radii up to 60 px
anns, centres = [], []
for i in range(n):
    cx, cy = rng.uniform(70, size - 70, 2)
    k = rng.randint(4, 12)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    r = rng.uniform(8, 60, k)
    pts = np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 2)
    anns.append({"segmentation": [[float(v) for v in pts]], "category_id": int(i % 2), "iscrowd": 0, "area": float(rng.uniform(100, 9000)),
                 "bbox": [float(cx - 60), float(cy - 60), float(cx + 60), float(cy + 60)], "bbox_mode": "XYXY_ABS"})
    centres.append((cx, cy))
rec = {"file_name": "synthetic.png", "image_id": 0, "height": size, "width": size, "annotations": anns}

# detections: one noisy blob near every annotation, packed on the host into rooms that are their tight boxes
rooms, words, areas = [], [], []
for cx, cy in centres:
    h, w = rng.randint(16, 120), rng.randint(16, 120)
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
classes = [int(v) for v in rng.randint(0, 2, n)]
forms = {"planes": planes, "crops": cset}
input_bytes = {"planes": planes.numel() * 4, "crops": cset.words * 4 + n * 36}
ids = {0: 0, 1: 1}

runs_by = {f: [] for f in forms}
digest = {}
for rep in range(reps):
    for form, packed in forms.items():                   # alternating: planes, crops, planes, crops, ...
        tables = {"bbox": CE.EvalTables(), "segm": CE.EvalTables()}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        rows = _score_pipeline_image(ops, rec, (size, size), packed, scores, classes, tabs, tables, ids)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        peak = int(torch.cuda.max_memory_allocated()) - before
        h = hashlib.sha256((repr(rows) + repr([tables[t].cat(k).tolist() for t in tables for k in ("iou", "d_area", "g_area")])).encode()).hexdigest()
        digest.setdefault(form, h)
        assert digest[form] == h, "a repetition gave other rows"
        runs_by[form].append(dict(seconds=dt, peak_bytes_above_input=peak))
        print(f"rep {rep} {form:6s}: {dt:.3f} s, {len(rows['instances'])} instances x {len(anns)} annotations, peak {peak / 2**20:.1f} MiB above its input "
              f"({input_bytes[form] / 2**20:.1f} MiB)", flush=True)

res = {"image": f"{size}x{size}", "instances": n, "annotations": len(anns), "reps_per_scorer": reps, "order": "alternating planes, crops",
       "same_rows": len(set(digest.values())) == 1, "row_digest": digest, "device": torch.cuda.get_device_name(0), "scorers": {}}
for form, rr in runs_by.items():
    steady = [r["seconds"] for r in rr[1:]]
    res["scorers"][form] = dict(first_image_seconds=rr[0]["seconds"], steady_seconds=steady,
                                steady_median_seconds=statistics.median(steady) if steady else None,
                                steady_min_max_seconds=[min(steady), max(steady)] if steady else None,
                                input_bytes=int(input_bytes[form]), peak_bytes_above_input=max(r["peak_bytes_above_input"] for r in rr))
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res))
