"""A/B of `inference_settings.mask_frame`: ONE synthetic 8192 x 8192 image (16 tiles of 2048, overlap 0, upscale 1, R101 -- the shape of
scripts/gpu_c3_large_image.py and of bench.py's one_8192_image leg) through the CLI's per-image path -- `final_instances` (class passes,
tile placement, 0.4 merges, 0.7 cross-class pass, spatial constraints), the RLE texts and `measure_image` -- REPS times per frame in one
process, the frames alternating (full, crop, full, crop, ...; the fourth argument names other frames to alternate, e.g.
full,crop,crop_direct), same models, same image, same box.  A frame written as ``<frame>+shape`` runs with
`inference_settings.shape_descriptors: true` (e.g. crop_direct,crop_direct+shape: the setting off and on, alternating), one written
as ``<frame>+inscribed`` with `inference_settings.inscribed_descriptors: true`, one written as ``<frame>+skeleton`` with
`inference_settings.skeleton_descriptors: true` -- any family of `maskset.FAMILIES`; several suffixes may follow one frame.  The suffix
``+neighbours`` runs with `inference_settings.neighbour_statistics: true` (the neighbour stage of `measure_image`; a radius of 50
pixels): its rows are counted and digested apart (`neighbour_rows`, `neighbour_rows_sha256`).  The suffix ``+agglomerates`` runs with
`inference_settings.agglomerate_statistics: true` (the agglomerate stage of `measure_image`, touching links across classes): its rows
are counted and digested apart too, with the number of components and the largest; ``+neighbours+agglomerates`` runs both, the second
on the first's border points (one border launch per image).

Per frame: the first image's time and the steady-state times apart (host clock around work that ends in a device synchronise; the
forwards are re-run every repetition, as a folder of such images would), the peak device memory of a repetition
(`torch.cuda.max_memory_allocated` after `reset_peak_memory_stats`), the device-to-host waits of the post-processing (the pipeline's
own counter) and every `Tensor.cpu()` / `Tensor.item()` call of the image (counted here: `measure_image`'s waits are among them; a
fetch that meets a mask with more contours than slots falls back to on-demand launches with copies of their own, counted apart), the
most full-frame planes alive after the tile mapping, whether all frames wrote the same rows (their 20 reference columns) and texts, and
a digest of ALL columns of the rows (`rows_sha256`: what pins the descriptor columns from one commit to the next).

    python scripts/gpu_crop_frame_ab.py [size=8192] [reps=4] [out.json] [frames=full,crop]
"""
import hashlib, json, os, statistics, sys, tempfile, time, types
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np, torch
import test_gpu_pipeline_e2e as T
from deepemia_amd import synth

size = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
out_path = Path(sys.argv[3]).resolve() if len(sys.argv) > 3 else ROOT / "profiles" / f"crop_frame_ab_{size}.json"
frames = tuple(sys.argv[4].split(",")) if len(sys.argv) > 4 else ("full", "crop")
tile = min(2048, size)
root = Path(tempfile.mkdtemp())
spatial = {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5,
           "overlap_rules": {0: {"allow_overlap": False, "max_iou_threshold": 0.3}, 1: {"allow_overlap": False, "max_iou_threshold": 0.5}}}
ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                  "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6, "min_size": 25},
                                                              "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5, "min_size": 5}},
                                  "tile_settings": {"tile_size": tile, "overlap_ratio": 0.0, "upscale_factor": 1.0, "edge_filter_enabled": True},
                                  "spatial_constraints": spatial}}
cfgdir, split, sds, _ = T._write_tree(root, [101], 0.5, 6.0, 0, 512, ds_cfg)
os.environ["DEEPEMIA_CONFIG_DIR"] = str(cfgdir); os.environ["DEEPEMIA_OFFLINE"] = "1"
os.chdir(root)

from deepemia_amd.engine import MaskRCNNEngine
from deepemia_amd.functions import inference as I
from deepemia_amd.maskset import ContourSet, families
from deepemia_amd.predictor import Predictor
from deepemia_amd.utils.mask_utils import rle_crop_launch, rle_text_from_payload
from deepemia_amd.utils.spatial_constraints import load_spatial_constraints

k = size // tile
img = np.concatenate([np.concatenate([synth.em_tile(100 + 4 * r + c, tile) for c in range(k)], axis=1) for r in range(k)], axis=0)
dev = "cuda:0"
image_dev = torch.from_numpy(img).to(dev)
st = I.PipelineSettings(T.DATASET)
pred = Predictor(MaskRCNNEngine(sds[101], 101, len(T.CLASSES), 0.3, dev, "f16x2"))
spatial_cfg = load_spatial_constraints(T.DATASET)
metadata = types.SimpleNamespace(thing_classes=T.CLASSES)
pipes = {f: I.InferencePipeline([pred], T.DATASET, dict(st.inf, mask_frame=f.split("+")[0]), st.global_config) for f in frames}
descriptors = {f: tuple(fam.name for fam in families([x for x in f.split("+")[1:] if x not in ("neighbours", "agglomerates")])) for f in frames}      # (an unknown suffix: ValueError)
neighbours = {f: "neighbours" in f.split("+")[1:] for f in frames}
agglomerates = {f: "agglomerates" in f.split("+")[1:] for f in frames}
NEIGHBOUR_RADIUS = 50.0
host_copies = [0]
for _name in ("cpu", "item"):
    def _counted(self, *a, _orig=getattr(torch.Tensor, _name), **k):
        host_copies[0] += bool(self.is_cuda)
        return _orig(self, *a, **k)
    setattr(torch.Tensor, _name, _counted)
fallbacks = [0]                      # fetches that met a mask with more contours than slots: measurements (shape, inscribed, skeleton values) on demand
def _fetch(self, *a, _orig=ContourSet.fetch, **k):
    out = _orig(self, *a, **k)
    fallbacks[0] += self.max_count > min(self._mslots, self.C)
    return out
ContourSet.fetch = _fetch
small = I.determine_small_classes(pipes[frames[0]].calculate_average_mask_sizes([("big.tif", image_dev)]), 50)
pipes[frames[0]].drop_cached("big.tif")


def one_image(pipe, descriptors=(), with_neighbours=False, with_agglomerates=False):
    """process_image of run_inference for this image: instances, RLE texts, measurement rows (and the neighbour / agglomerate rows)."""
    name = "big.tif"
    pipe.begin_image_stats()
    packed, scores, classes, tabs = I.final_instances(pipe, st, name, image_dev, small, len(T.CLASSES), spatial_cfg, I.image_phases_enabled(pipe))
    n = 0 if packed is None else int(packed.shape[0])
    result = {"masks": packed, "scores": scores, "classes": classes, "hw": (size, size),
              "area": None if tabs is None else tabs[0], "bbox": None if tabs is None else tabs[1]}
    if n and pipe.crop:
        crop = (packed.payload[:packed.words], packed.room_h, packed.offsets_h)
    else:
        crop = rle_crop_launch(pipe.ops, packed, tabs[0], tabs[1]) if n else None
    extra = [crop[0]] if crop is not None else None
    statistics = {"neighbours": I.NeighbourSetting(with_neighbours, NEIGHBOUR_RADIUS), "agglomerates": I.AgglomerateSetting(with_agglomerates, None, "any")}
    rows, stat_rows = I.measure_image(pipe.ops, name, result, str(root), str(split), metadata, T.DATASET, False, False, image_dev=image_dev,
                                      extra=extra, note_planes=pipe._note_planes, crop_direct=pipe.crop_direct, descriptors=descriptors,
                                      statistics=statistics)
    texts = rle_text_from_payload(extra[0], crop[1], crop[2], size) if crop is not None else []
    if with_neighbours and pipe.crop:      # (a crop-framed set is a few MiB: keeping it does not move the next repetition's peak)
        last_set[pipe.mask_frame] = (pipe, packed, classes, tabs)
    if with_agglomerates and pipe.crop:
        last_agg[pipe.mask_frame] = (pipe, packed, classes, tabs)
    pipe.drop_cached(name)
    return n, rows, texts, pipe.end_image_stats((size, size)), stat_rows.get("neighbours"), stat_rows.get("agglomerates")


last_set = {}                        # crop frame -> the final set of the last image measured with +neighbours
last_agg = {}                        # ... and with +agglomerates
digest_ag = {}
runs = {f: [] for f in pipes}
digest, digest_all, digest_nb = {}, {}, {}          # per frame: texts + the 20 reference columns; ALL columns of the rows; the neighbour rows
for rep in range(reps):
    for frame, pipe in pipes.items():                    # alternating: full, crop, full, crop, ... (the order of `frames`)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        w0, c0, f0 = pipe.d2h_waits, host_copies[0], fallbacks[0]
        t0 = time.perf_counter()
        n, rows, texts, stats, nrows, arows = one_image(pipe, descriptors[frame], neighbours[frame], agglomerates[frame])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert all(len(r) == 20 + sum(len(I.DESCRIPTOR_CSV[name][0]) for name in descriptors[frame]) for r in rows)
        h = hashlib.sha256(("\n".join(texts) + repr([r[:20] for r in rows])).encode()).hexdigest()
        h_all = hashlib.sha256(repr(rows).encode()).hexdigest()
        digest.setdefault(frame, h)
        digest_all.setdefault(frame, h_all)
        h_nb = None if nrows is None else hashlib.sha256(repr(nrows).encode()).hexdigest()
        digest_nb.setdefault(frame, h_nb)
        h_ag = None if arows is None else hashlib.sha256(repr(arows).encode()).hexdigest()
        digest_ag.setdefault(frame, h_ag)
        assert digest[frame] == h and digest_all[frame] == h_all and digest_nb[frame] == h_nb and digest_ag[frame] == h_ag, "a repetition wrote other rows"
        runs[frame].append(dict(seconds=dt, peak_bytes=int(torch.cuda.max_memory_allocated()), d2h_waits=pipe.d2h_waits - w0,
                                host_copies=host_copies[0] - c0, fetch_fallbacks=fallbacks[0] - f0, instances=n,
                                rows=len(rows), neighbour_rows=None if nrows is None else len(nrows),
                                agglomerate_rows=None if arows is None else len(arows), largest_agglomerate=None if not arows else max(r[1] for r in arows),
                                full_frame_planes_peak=stats["full_frame_planes_peak"]))
        print(f"rep {rep} {frame:11s}: {dt:.3f} s, {n} instances, {len(rows)} rows, peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB, "
              f"{pipe.d2h_waits - w0} waits, {host_copies[0] - c0} device-to-host copies ({fallbacks[0] - f0} fetch fallbacks), {stats['full_frame_planes_peak']} planes", flush=True)

res = {"image": f"{size}x{size}", "tiles": k * k, "tile": tile, "model": "R101 f16x2", "reps_per_frame": reps, "order": "alternating " + ", ".join(frames),
       "same_rows_and_texts": len(set(digest.values())) == 1, "same_neighbour_rows": len({v for v in digest_nb.values() if v is not None}) <= 1,
       "same_agglomerate_rows": len({v for v in digest_ag.values() if v is not None}) <= 1, "device": torch.cuda.get_device_name(0), "frames": {}}
for frame, rr in runs.items():
    steady = [r["seconds"] for r in rr[1:]]
    res["frames"][frame] = dict(first_image_seconds=rr[0]["seconds"], steady_seconds=steady,
                                steady_median_seconds=statistics.median(steady) if steady else None,
                                steady_min_max_seconds=[min(steady), max(steady)] if steady else None,
                                peak_bytes_first=rr[0]["peak_bytes"], peak_bytes_steady=max(r["peak_bytes"] for r in rr[1:]) if steady else None,
                                d2h_waits_per_image=rr[-1]["d2h_waits"], host_copies_per_image=rr[-1]["host_copies"], fetch_fallbacks_per_image=rr[-1]["fetch_fallbacks"], instances=rr[-1]["instances"], rows=rr[-1]["rows"],
                                rows20_texts_sha256=digest[frame], rows_sha256=digest_all[frame],
                                neighbour_rows=rr[-1]["neighbour_rows"], neighbour_rows_sha256=digest_nb[frame],
                                agglomerate_rows=rr[-1]["agglomerate_rows"], largest_agglomerate=rr[-1]["largest_agglomerate"],
                                agglomerate_rows_sha256=digest_ag[frame],
                                full_frame_planes_peak=max(r["full_frame_planes_peak"] for r in rr))


def stage_alone(frame):
    """The neighbour stage by itself on the last final set of ``frame``: device time of its two launches (events, 5 runs, the
    median), for all masks and with the masks of the longest borders left out -- a launch that ends on one slow mask gets much
    shorter without it."""
    pipe, packed, classes, tabs = last_set[frame]
    area, group = np.asarray(tabs[0]), np.asarray(classes, dtype=np.int32)
    r2 = I.neighbour_r2(NEIGHBOUR_RADIUS, 1.0)

    def timed(keep):
        sub = packed if keep is None else packed.select(keep)
        call = lambda: sub.neighbours(area=area if keep is None else area[keep], group=group if keep is None else group[keep], r2=r2)
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            nb = call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), nb
    t_all, nb = timed(None)
    nborder = nb.nborder.cpu().numpy().astype(np.int64)
    order = np.argsort(-nborder, kind="stable")
    out = dict(masks=int(len(nborder)), device_ms_all=t_all, border_points=int(nborder.sum()), border_points_max=int(nborder.max()),
               border_points_median=float(np.median(nborder)), border_points_above_lds_limit=int((nborder > 8192).sum()))
    for drop in (1, 8):
        out[f"device_ms_without_{drop}_longest"] = timed(np.sort(order[drop:]))[0]
    return out


def agglomerate_stage_alone(frame):
    """The agglomerate stage by itself on the last final set of ``frame``: device time (events, 5 runs, the median) of its four
    launches, of the three behind a neighbour stage's border points, and of all four with the masks of the longest borders or of the
    most links left out -- a launch that ends on one slow workgroup gets much shorter without it."""
    pipe, packed, classes, tabs = last_agg[frame]
    area = np.asarray(tabs[0])

    def timed(keep, border=False):
        sub = packed if keep is None else packed.select(keep)
        a = area if keep is None else area[keep]
        nb = sub.neighbours(area=a, r2=-1) if border else None
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ag = sub.agglomerates(area=a, l2=2, border=nb)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), ag
    t_all, ag = timed(None)
    nborder, degree, label = (t.cpu().numpy().astype(np.int64) for t in (ag.nborder, ag.degree, ag.label))
    sizes = np.bincount(label[label >= 0])
    out = dict(masks=int(len(label)), device_ms_all=t_all, device_ms_border_reused=timed(None, border=True)[0], components=int((sizes > 0).sum()),
               largest_component=int(sizes.max()), singletons=int((sizes == 1).sum()), links=int(degree.sum() // 2), degree_max=int(degree.max()),
               border_points_max=int(nborder.max()), link_matrix_bytes=int(ag.links.numel() * 4))
    for what, order in (("longest_borders", np.argsort(-nborder, kind="stable")), ("most_linked", np.argsort(-degree, kind="stable"))):
        for drop in (1, 8):
            out[f"device_ms_without_{drop}_{what}"] = timed(np.sort(order[drop:]))[0]
    return out


if last_set:
    res["neighbour_stage_alone"] = {f: stage_alone(f) for f in last_set}
if last_agg:
    res["agglomerate_stage_alone"] = {f: agglomerate_stage_alone(f) for f in last_agg}
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text(json.dumps(res, indent=1))
print(json.dumps(res))
