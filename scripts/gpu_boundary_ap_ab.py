"""A/B of `evaluation.boundary_ap`: the scoring of the synthetic 8192 x 8192 image of `gpu_eval_frame_ab.py` (roughly 900 final
instances as noisy blobs of up to 120 px, 900 polygon annotations of up to 120 px) through both scorers of the evaluate task's
pipeline mode -- `planes` and `crops` -- with the boundary task OFF (the parent's behaviour: nothing of it is launched), ON at the
default ratio (d = 232 at this size: every one of these particles is narrower than 2d + 1 = 465 px, so each band is its mask,
copied and counted) and ON at `boundary_width: 8` (the erosion passes do run).  One first repetition and REPS steady ones per
(scorer, setting), all alternating in one process, same inputs, same box.  No model runs; the figures are the scoring alone
(`_score_pipeline_image`, host clock around work that ends in a device synchronise).

    python scripts/gpu_boundary_ap_ab.py [size=8192] [n=900] [reps=3] [out.json]
"""
import json, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np, torch
from deepemia_amd import cocoeval as CE
from deepemia_amd.cropset import CropMaskSet
from deepemia_amd.functions.evaluate_model import _new_tables, _score_pipeline_image
from deepemia_amd.maskset import MaskOps

size = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
n = int(sys.argv[2]) if len(sys.argv) > 2 else 900
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_path = Path(sys.argv[4]).resolve() if len(sys.argv) > 4 else ROOT / "profiles" / f"boundary_ap_ab_{size}.json"
ops = MaskOps("cuda:0")
rng = np.random.RandomState(8)

# the image of gpu_eval_frame_ab.py: concave rings with radii up to 60 px, one noisy blob near each
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
settings = {"off": None, "on_default_ratio": (CE.BOUNDARY_RATIO, None), "on_width_8": (CE.BOUNDARY_RATIO, 8)}
ids = {0: 0, 1: 1}

runs_by = {(f, s): [] for f in forms for s in settings}
iou_of = {}
for rep in range(reps + 1):
    for form, packed in forms.items():                   # alternating: every (scorer, setting) once per round
        for name, boundary in settings.items():
            tables = _new_tables(boundary)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            rows = _score_pipeline_image(ops, rec, (size, size), packed, scores, classes, tabs, tables, ids, boundary=boundary)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            peak = int(torch.cuda.max_memory_allocated()) - before
            iou_of[form, name] = {t: tables[t].cat("iou") for t in tables}
            runs_by[form, name].append(dict(seconds=dt, peak_bytes_above_input=peak))
            print(f"rep {rep} {form:6s} {name:16s}: {dt:.3f} s, peak {peak / 2**20:.1f} MiB above its input", flush=True)

d_default = CE.boundary_width(size, size)
res = {"image": f"{size}x{size}", "instances": n, "annotations": len(anns), "steady_reps": reps, "order": "alternating scorers and settings",
       "default_width_px": d_default, "device": torch.cuda.get_device_name(0),
       "segm_iou_same_in_every_run": all(np.array_equal(v["segm"], iou_of["planes", "off"]["segm"]) for v in iou_of.values()),
       "boundary_iou_same_in_both_frames": all(np.array_equal(iou_of["planes", s]["boundary"], iou_of["crops", s]["boundary"])
                                               for s in settings if settings[s] is not None),
       "boundary_equals_segm_at_default_ratio": bool(np.array_equal(iou_of["crops", "on_default_ratio"]["boundary"], iou_of["crops", "off"]["segm"])),
       "pairs_where_boundary_is_below_segm_at_width_8": int(np.count_nonzero(iou_of["crops", "on_width_8"]["boundary"] < iou_of["crops", "off"]["segm"])),
       "runs": {}}
for (form, name), rr in runs_by.items():
    steady = [r["seconds"] for r in rr[1:]]
    res["runs"][f"{form}/{name}"] = dict(first_seconds=rr[0]["seconds"], steady_seconds=steady, steady_median_seconds=statistics.median(steady),
                                         steady_min_max_seconds=[min(steady), max(steady)],
                                         peak_bytes_above_input=max(r["peak_bytes_above_input"] for r in rr))
for form in forms:
    off = res["runs"][f"{form}/off"]["steady_median_seconds"]
    for name in settings:
        if settings[name] is not None:
            res["runs"][f"{form}/{name}"]["steady_median_over_off"] = res["runs"][f"{form}/{name}"]["steady_median_seconds"] / off
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res))
