"""Dev script: the ranks' exchange in both forms on BASELINE configs[2]'s shape -- a folder of N identical-size SIZE x SIZE images
(16 tiles of SIZE / 4, overlap 0, upscale 1, R101) through `main.py --task inference` with TWO ranks on ONE GPU (gloo,
DEEPEMIA_SHARD=tiles), `mask_frame: full` (the plane exchange) against `mask_frame: crop_direct` + `rank_exchange: crops`,
alternating, every run in fresh processes.  Per image: the seconds of `final_instances` (class passes, exchange, merges,
constraints; device synchronised) on every rank; per rank the peak device memory; per run the SHA-256 of both CSVs.

    python scripts/gpu_rank_exchange_ab.py [SIZE=8192] [IMAGES=3] [REPEATS=2] [OUT=profiles/rank_exchange_ab_SIZE.json]"""
import hashlib
import json
import os
import socket
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FORMS = {"planes": {"mask_frame": "full"}, "crops": {"mask_frame": "crop_direct", "rank_exchange": "crops"}}
DATASET = "synthpores"


def _worker(rank, world, port, root, cfgdir, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      DEEPEMIA_DIST_BACKEND="gloo", DEEPEMIA_CONFIG_DIR=str(cfgdir), DEEPEMIA_OFFLINE="1", DEEPEMIA_LOG_DIR=str(root),
                      DEEPEMIA_SHARD="tiles", DEEPEMIA_ONE_DEVICE="1", DEEPEMIA_WORKERS="1")
    os.chdir(root)
    import torch
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    import main as cli
    from deepemia_amd.functions import inference as INF

    orig, times = INF.final_instances, []

    def timed(pipe, st, name, *a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            return orig(pipe, st, name, *a, **k)
        finally:
            torch.cuda.synchronize()
            times.append((name, time.perf_counter() - t0, pipe.d2h_waits))

    INF.final_instances = timed
    t0 = time.perf_counter()
    rc = cli.main(["--task", "inference", "--dataset_name", DATASET, "--threshold", "0.3", "--no-gpu-check"])
    out[rank] = dict(rc=rc, wall_s=time.perf_counter() - t0, images=[(n, round(t, 4), w) for n, t, w in times],
                     peak_gib=torch.cuda.max_memory_allocated() / 2**30, stats=dict(INF.LAST_RUN_STATS))


def main():
    import numpy as np
    import torch.multiprocessing as mp
    import yaml
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    import test_gpu_pipeline_e2e as T
    from deepemia_amd import synth

    size = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    n_images = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    out_path = Path(sys.argv[4] if len(sys.argv) > 4 else ROOT / "profiles" / f"rank_exchange_ab_{size}.json")
    tile = size // 4
    root = Path(tempfile.mkdtemp())
    spatial = {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5,
               "overlap_rules": {0: {"allow_overlap": False, "max_iou_threshold": 0.3}, 1: {"allow_overlap": False, "max_iou_threshold": 0.5}}}
    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6, "min_size": 25},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5, "min_size": 5}},
                                      "tile_settings": {"tile_size": tile, "overlap_ratio": 0.0, "upscale_factor": 1.0, "edge_filter_enabled": True},
                                      "spatial_constraints": spatial}}
    cfgdir, split, _, _ = T._write_tree(root, [101], 0.5, 6.0, 0, 512, ds_cfg)
    inf = root / "DATASET" / "INFERENCE"
    for k in range(n_images):
        rows = [[synth.em_tile(100 + 16 * k + 4 * r + c, tile) for c in range(4)] for r in range(4)]
        img = np.concatenate([np.concatenate(row, axis=1) for row in rows], axis=0)
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(inf / f"big_{k}.tif")
    runs = []
    for rep in range(repeats):
        for form, settings in FORMS.items():
            cfg = json.loads(json.dumps(ds_cfg))
            cfg["inference_overrides"].update(settings)
            (cfgdir / "datasets" / f"{DATASET}.yaml").write_text(yaml.safe_dump(cfg, sort_keys=False))
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
            s.close()
            out = mp.Manager().dict()
            mp.spawn(_worker, args=(2, port, str(root), str(cfgdir), out), nprocs=2, join=True)
            sha = hashlib.sha256((split / "measurements_results.csv").read_bytes() + (split / "R50_flip_results.csv").read_bytes()).hexdigest()
            n_rows = len((split / "measurements_results.csv").read_text().splitlines()) - 1
            runs.append(dict(form=form, repeat=rep, rows=n_rows, sha256=sha, ranks={int(r): v for r, v in out.items()}))
            print(json.dumps(runs[-1]), flush=True)
    rec = dict(size=size, images=n_images, tile=tile, ranks=2, backend="gloo, both ranks on one device", runs=runs,
               same_bytes=len({r["sha256"] for r in runs}) == 1)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(rec, indent=1))
    print("same bytes in every run:", rec["same_bytes"])


if __name__ == "__main__":
    main()
