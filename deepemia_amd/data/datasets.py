"""Dataset registration kept as a drop-in (reference ``src/data/datasets.py:65-153,242-258``).

Only the parts the inference path consumes are reproduced: ``read_dataset_info`` and the
``thing_classes`` metadata that ``register_datasets`` attaches to ``<dataset>_train`` /
``<dataset>_test`` (``inference.py:599-603``).  The training dicts the reference loads and discards
(``inference.py:598,607``) are registered as a lazy no-op; the train/test split and the custom-JSON
-> Detectron2 dict conversion are training-side and out of scope.
"""
from __future__ import annotations

import json
from types import SimpleNamespace
from typing import Callable, Dict

from ..utils.logger_utils import system_logger


class _Metadata(SimpleNamespace):
    def set(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)
        return self

    def get(self, key, default=None):
        return getattr(self, key, default)


class _MetadataCatalog:
    """``detectron2.data.MetadataCatalog`` work-alike: ``get(name)`` creates on first use."""

    def __init__(self):
        self._m: Dict[str, _Metadata] = {}

    def get(self, name: str) -> _Metadata:
        if name not in self._m:
            self._m[name] = _Metadata(name=name)
        return self._m[name]

    def list(self):
        return list(self._m)

    def remove(self, name):
        self._m.pop(name, None)


class _DatasetCatalog:
    """``detectron2.data.DatasetCatalog`` work-alike (lazy callables)."""

    def __init__(self):
        self._d: Dict[str, Callable] = {}

    def register(self, name: str, func: Callable) -> None:
        self._d[name] = func

    def get(self, name: str):
        if name not in self._d:
            raise KeyError(f"Dataset '{name}' is not registered! Available datasets are: {', '.join(self._d)}")
        return self._d[name]()

    def list(self):
        return list(self._d)

    def remove(self, name):
        self._d.pop(name, None)


MetadataCatalog = _MetadataCatalog()
DatasetCatalog = _DatasetCatalog()


def read_dataset_info(file_path) -> dict:
    """``{name: (img_dir, label_dir, [classes])}`` from ``dataset_info.json`` (``datasets.py:242-258``)."""
    with open(file_path, "r") as f:
        data = json.load(f)
    info = {k: tuple(v) if isinstance(v, list) else v for k, v in data.items()}
    system_logger.info(f"Dataset Info: {info}")
    return info


def register_datasets(dataset_info, dataset_name, test_size=0.2, dataset_format="json"):
    """Make ``MetadataCatalog.get(f"{dataset_name}_train").thing_classes`` available
    (``datasets.py:65-153``).  Raises ``ValueError`` for an unknown dataset / format, as the reference."""
    if dataset_format not in ("json", "coco"):
        raise ValueError(f"Unknown dataset_format: {dataset_format}")
    if dataset_name not in dataset_info:
        raise ValueError(f"Dataset '{dataset_name}' not found in dataset_info.")
    _img_dir, _label_dir, thing_classes = dataset_info[dataset_name]
    for split in ("train", "test"):
        DatasetCatalog.register(f"{dataset_name}_{split}", lambda: [])  # training dicts: not needed for inference
        MetadataCatalog.get(f"{dataset_name}_{split}").set(thing_classes=list(thing_classes))
    system_logger.info(f"Registered dataset '{dataset_name}' ({dataset_format}) with classes {list(thing_classes)}")


# ---- the test split for the evaluate task (reference datasets.py:36-62, 108-133, 156-239) ------------------------------------
def split_rule(files, test_size: float = 0.2, seed: int = 42):
    """``sklearn.model_selection.train_test_split(files, test_size=test_size, random_state=seed)``: ``n_test = ceil(test_size *
    n)``, ``perm = RandomState(seed).permutation(n)``, test = ``perm[:n_test]``, train = ``perm[n_test:]``.
    Returns ``(train, test)``."""
    import math

    import numpy as np

    files = list(files)
    n = len(files)
    n_test = int(math.ceil(test_size * n))
    perm = np.random.RandomState(seed).permutation(n)
    return [files[i] for i in perm[n_test:]], [files[i] for i in perm[:n_test]]


def load_or_create_split(img_dir, dataset_name: str, split_dir, test_size: float = 0.2) -> dict:
    """``<split_dir>/<name>_split.json`` when it exists; otherwise the split of the ``.json`` label files listed in ``img_dir``
    by :func:`split_rule`, written there.  The listing is SORTED by name (the reference splits ``os.listdir`` order, which
    depends on the file system), so the same folder always gives the same split."""
    import os

    split_file = os.path.join(str(split_dir), f"{dataset_name}_split.json")
    if os.path.exists(split_file):
        with open(split_file) as f:
            return json.load(f)
    files = sorted(f for f in os.listdir(img_dir) if f.endswith(".json"))
    train, test = split_rule(files, test_size=test_size)
    os.makedirs(str(split_dir), exist_ok=True)
    data = {"train": train, "test": test}
    with open(split_file, "w") as f:
        json.dump(data, f)
    system_logger.info(f"Split created and saved at {split_file}")
    return data


def ellipse_polygon(cx: float, cy: float, rx: float, ry: float, angle: float):
    """``shapely.affinity.rotate(shapely.affinity.scale(Point(c).buffer(1), int(rx), int(ry)), angle).exterior.coords``
    restated without shapely: the 64-gon of a buffered point (first vertex at angle 0, then clockwise in x-right / y-up
    terms, angle -2*pi*k/64, and the first vertex again to close the ring: 65 points), scaled about its box centre, then
    rotated by ``angle`` degrees about the new box centre -- shapely's affine matrices, term by term.  Returns (px, py)."""
    import math

    import numpy as np

    th = np.arange(64) * (2.0 * math.pi / 64)
    px = cx + 1.0 * np.cos(-th)
    py = cy + 1.0 * np.sin(-th)
    px, py = np.append(px, px[0]), np.append(py, py[0])
    sx, sy = int(rx), int(ry)
    x0, y0 = (px.min() + px.max()) / 2.0, (py.min() + py.max()) / 2.0
    px, py = sx * px + 0.0 * py + (x0 - x0 * sx), 0.0 * px + sy * py + (y0 - y0 * sy)
    a = angle * math.pi / 180.0
    cosp, sinp = math.cos(a), math.sin(a)
    cosp = 0.0 if abs(cosp) < 2.5e-16 else cosp
    sinp = 0.0 if abs(sinp) < 2.5e-16 else sinp
    x0, y0 = (px.min() + px.max()) / 2.0, (py.min() + py.max()) / 2.0
    xoff, yoff = x0 - x0 * cosp + y0 * sinp, y0 - x0 * sinp - y0 * cosp
    return cosp * px + -sinp * py + xoff, sinp * px + cosp * py + yoff


def polygon_area(poly) -> float:
    """Detectron2's ``PolygonMasks.area`` of one instance (shoelace per polygon, summed, as float32)."""
    import numpy as np

    total = 0.0
    for p in poly:
        p = np.asarray(p, dtype=np.float64)
        x, y = p[0::2], p[1::2]
        total += 0.5 * np.abs(np.dot(x, np.roll(y, 1)) - np.dot(y, np.roll(x, 1)))
    return float(np.float32(total))


def get_split_dicts(img_dir, label_dir, files, thing_classes):
    """The reference's ``get_split_dicts`` (``datasets.py:156-239``): one record per label file, ``image_id`` = its index in
    ``files``; polygons from the ``points`` pairs and ellipses as :func:`ellipse_polygon`, +0.5 on every coordinate of the
    segmentation, ``bbox`` = XYXY min / max of the unshifted coordinates; unknown class names skipped with a warning.
    ``area`` (Detectron2's ``convert_to_coco_dict``: the shoelace area) and ``iscrowd`` = 0 are added for the scorer."""
    import os

    import numpy as np

    name_to_id = {name: i for i, name in enumerate(thing_classes)}
    out = []
    for idx, file in enumerate(files):
        with open(os.path.join(str(label_dir), file)) as f:
            anns = json.load(f)
        rec = {"file_name": os.path.join(str(img_dir), anns["metadata"]["name"]), "image_id": idx,
               "height": anns["metadata"]["height"], "width": anns["metadata"]["width"]}
        objs = []
        for anno in anns["instances"]:
            kind = anno["type"]
            if kind == "ellipse":
                px, py = ellipse_polygon(anno["cx"], anno["cy"], anno["rx"], anno["ry"], anno["angle"])
                px, py = list(px), list(py)
            elif kind == "polygon":
                pts = anno["points"]
                px, py = list(pts[0:-1:2]), list(pts[1:-1:2])
                px.append(pts[0])
                py.append(pts[-1])
            else:
                system_logger.warning(f"Unknown annotation type: {kind}")
                continue
            poly = [c for x, y in zip(px, py) for c in (x + 0.5, y + 0.5)]
            if anno["className"] not in name_to_id:
                system_logger.warning(f"Category Name Not Found: {anno['className']}")
                continue
            objs.append({"bbox": [np.min(px), np.min(py), np.max(px), np.max(py)], "bbox_mode": "XYXY_ABS",
                         "segmentation": [poly], "category_id": name_to_id[anno["className"]],
                         "area": polygon_area([poly]), "iscrowd": 0})
        rec["annotations"] = objs
        out.append(rec)
    return out


def load_coco_test(base_path):
    """``<base_path>/annotations/instances_test.json`` + ``<base_path>/test/`` as Detectron2's ``load_coco_json`` reads it:
    category ids mapped to contiguous ids in sorted-id order (``id_map`` = dataset id -> contiguous id), ``bbox`` XYWH,
    polygons (those with an even length >= 6 kept) or RLE (compressed string or uncompressed list) as in the file, ``iscrowd``
    honoured.  ``area`` is the file's when present, else Detectron2's ``convert_to_coco_dict`` rule (shoelace for polygons,
    pixel count for RLE, box area otherwise).  Returns (records, thing_classes, id_map)."""
    import os

    import numpy as np

    with open(os.path.join(str(base_path), "annotations", "instances_test.json")) as f:
        data = json.load(f)
    cats = sorted(data.get("categories", []), key=lambda c: c["id"])
    id_map = {c["id"]: i for i, c in enumerate(cats)}
    names = [c["name"] for c in cats]
    by_img = {}
    for a in data.get("annotations", []):
        by_img.setdefault(a["image_id"], []).append(a)
    recs = []
    for img in sorted(data.get("images", []), key=lambda r: r["id"]):
        objs = []
        for a in by_img.get(img["id"], []):
            seg = a.get("segmentation")
            obj = {"bbox": [float(v) for v in a["bbox"]], "bbox_mode": "XYWH_ABS", "category_id": id_map[a["category_id"]],
                   "iscrowd": int(a.get("iscrowd", 0))}
            if isinstance(seg, dict):
                obj["segmentation"] = seg
            elif isinstance(seg, list):
                seg = [p for p in seg if len(p) % 2 == 0 and len(p) >= 6]
                if not seg:
                    continue
                obj["segmentation"] = seg
            if "area" in a:
                obj["area"] = float(a["area"])
            elif isinstance(obj.get("segmentation"), list):
                obj["area"] = polygon_area(obj["segmentation"])
            elif isinstance(obj.get("segmentation"), dict):
                obj["area"] = float(rle_counts_of(obj["segmentation"])[1::2].sum())
            else:
                obj["area"] = float(np.float32(obj["bbox"][2]) * np.float32(obj["bbox"][3]))
            objs.append(obj)
        recs.append({"file_name": os.path.join(str(base_path), "test", img["file_name"]), "image_id": img["id"],
                     "height": img["height"], "width": img["width"], "annotations": objs})
    return recs, names, id_map


def rle_counts_of(seg: dict):
    """Run lengths of an RLE segmentation: ``counts`` a list (uncompressed) or a compressed string."""
    import numpy as np

    from ..cocoeval import rle_from_string

    c = seg["counts"]
    return np.asarray(c, dtype=np.int64) if isinstance(c, list) else rle_from_string(c if isinstance(c, str) else c.decode())
