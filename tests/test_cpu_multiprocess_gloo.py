"""CPU, world_size 2, gloo: the N > 1 path -- unit sharding and the all-gather of per-tile instance
tables -- gives every rank the same global table, in (unit id, detector order) order, bit-exact."""
import os
from pathlib import Path
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_unit(unit_id, h, w):
    rng = np.random.default_rng(1000 + unit_id)
    n = int(rng.integers(0, 5))
    masks = np.zeros((n, h, w), dtype=bool)
    for i in range(n):
        if rng.random() < 0.15:
            continue  # an empty mask
        y0, x0 = rng.integers(0, h - 8), rng.integers(0, w - 8)
        y1, x1 = rng.integers(y0 + 1, h + 1), rng.integers(x0 + 1, w + 1)
        masks[i, y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) > 0.4
    scores = rng.uniform(0.3, 1.0, n) * 0.6   # float64 (ensemble scores are score * weight products)
    classes = rng.integers(0, 2, n)
    return masks, scores, classes


def _pack(masks):
    m, h, w = masks.shape
    p = np.packbits(masks.reshape(m, h, w // 32, 32), axis=-1, bitorder="little").view(np.uint32).reshape(m, h, w // 32)
    return torch.from_numpy(p.view(np.int32).copy())


def _bbox_area(masks):
    bb = np.full((masks.shape[0], 4), -1, dtype=np.int64)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if len(ys):
            bb[i] = (ys.min(), xs.min(), ys.max(), xs.max())
    return bb, masks.sum((1, 2))


def _worker(rank, world, port, n_units, h, w, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deepemia_amd import parallel as PL

    mine = PL.shard_indices(n_units, rank, world)
    masks, scores, classes, units = [], [], [], []
    for u in mine:
        m, s, c = _make_unit(u, h, w)
        masks.append(m)
        scores += list(s)
        classes += list(c)
        units += [u] * len(s)
    masks = np.concatenate(masks) if masks else np.zeros((0, h, w), bool)
    bb, area = _bbox_area(masks)
    hdr, pay = PL.encode_instance_table(_pack(masks) if len(masks) else None, scores, classes, units, bb, area)
    gt = PL.all_gather_instance_tables(hdr, pay)
    packed, gs, gc, gu = PL.decode_instance_table(gt.header, gt.payload, h, w, host_header=gt.host_header, offsets=gt.offsets)
    out[rank] = (packed.numpy(), gs, gc, gu)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_units", [(2, 7), (2, 1)])
def test_all_gather_instance_tables_world2(world, n_units):
    h, w = 48, 96
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), n_units, h, w, out), nprocs=world, join=True)
    # expected global table: units in order, detector order inside a unit
    em, es, ec, eu = [], [], [], []
    for u in range(n_units):
        m, s, c = _make_unit(u, h, w)
        em.append(m)
        es += [float(v) for v in s]
        ec += [int(v) for v in c]
        eu += [u] * len(s)
    em = np.concatenate(em)
    exp_packed = _pack(em).numpy() if len(em) else np.zeros((0, h, w // 32), np.int32)
    for r in range(world):
        packed, gs, gc, gu = out[r]
        assert gu == eu and gc == ec and gs == es
        np.testing.assert_array_equal(packed, exp_packed)


def test_single_process_roundtrip_and_sharding():
    from deepemia_amd import parallel as PL

    assert PL.shard_indices(16, 3, 8) == [3, 11] and PL.shard_indices(5, 7, 8) == []
    assert sorted(sum((PL.shard_indices(16, r, 8) for r in range(8)), [])) == list(range(16))
    m, s, c = _make_unit(3, 64, 64)
    bb, area = _bbox_area(m)
    hdr, pay = PL.encode_instance_table(_pack(m) if len(m) else None, s, c, [5] * len(s), bb, area)
    gt = PL.all_gather_instance_tables(hdr, pay)          # not initialised -> local table, sorted
    packed, gs, gc, gu = PL.decode_instance_table(gt.header, gt.payload, 64, 64, host_header=gt.host_header, offsets=gt.offsets)
    np.testing.assert_array_equal(packed.numpy(), _pack(m).numpy() if len(m) else packed.numpy())
    assert gs == [float(v) for v in s] and gu == [5] * len(s)
    assert int(pay.numel()) * 4 < max(1, m.size // 8)           # cropped payload is smaller than the full frames


def _worker_capacity(rank, world, port, h, w, out):
    """Four exchanges in one job with tables of very different sizes: the agreed capacity is used when it fits (one
    collective, one host wait), outgrown once (every rank redoes that exchange exactly), and the result is always exact."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deepemia_amd import parallel as PL

    PL.reset_capacity()
    tables, log = [], []
    for step, n_units in enumerate((6, 5, 40, 3)):          # 40 units: far more rows than 1.5 x the previous maximum
        mine = PL.shard_indices(n_units, rank, world)
        masks, scores, classes, units = [np.zeros((0, h, w), bool)], [], [], []
        for u in mine:
            m, s, c = _make_unit(100 * step + u, h, w)
            masks.append(m)
            scores += list(s)
            classes += list(c)
            units += [u] * len(s)
        masks = np.concatenate(masks)
        bb, area = _bbox_area(masks)
        hdr, pay = PL.encode_instance_table(_pack(masks) if len(masks) else None, scores, classes, units, bb, area)
        before = dict(PL.stats)
        gt = PL.all_gather_instance_tables(hdr, pay)
        log.append((PL.stats["size_exchanges"] - before["size_exchanges"], PL.stats["host_syncs"] - before["host_syncs"]))
        packed, gs, gc, gu = PL.decode_instance_table(gt.header, gt.payload, h, w, host_header=gt.host_header, offsets=gt.offsets)
        tables.append((packed.numpy(), gs, gc, gu))
    out[rank] = (tables, log)
    dist.barrier()
    dist.destroy_process_group()


def test_agreed_capacity_exchange_is_exact_and_needs_one_host_wait_in_steady_state():
    h, w, world = 48, 96, 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_capacity, args=(world, _free_port(), h, w, out), nprocs=world, join=True)
    for step, n_units in enumerate((6, 5, 40, 3)):
        em, es, ec, eu = [np.zeros((0, h, w), bool)], [], [], []
        for u in range(n_units):
            m, s, c = _make_unit(100 * step + u, h, w)
            em.append(m)
            es += [float(v) for v in s]
            ec += [int(v) for v in c]
            eu += [u] * len(s)
        exp = _pack(np.concatenate(em)).numpy()
        for r in range(world):
            packed, gs, gc, gu = out[r][0][step]
            assert gu == eu and gc == ec and gs == es
            np.testing.assert_array_equal(packed, exp)
    for r in range(world):
        log = out[r][1]
        assert log[0] == (1, 2)            # first exchange of a job: sizes first
        assert log[1] == (0, 1)            # fits the agreed capacity: ONE collective, ONE host wait
        assert log[2] == (1, 3)            # outgrown: detected from the gathered sizes, redone exactly by every rank
        assert log[3] == (0, 1)
    assert out[0][1] == out[1][1]


def test_bench_gpus_n_starts_its_ranks_itself_and_refuses_a_wrong_world_size():
    """``python bench.py --gpus N`` is the form of the driver's command: with N > 1 and no WORLD_SIZE the process becomes a launcher
    (a child ``torch.distributed.run`` with N ranks, its stdout = rank 0's one JSON line, never a GPU call of its own); a WORLD_SIZE
    that differs from --gpus is refused with exit code 2 instead of being reported as N.  ``--rendezvous-only`` stops the
    processes after their rendezvous (gloo), so the role logic runs on a CPU box -- including the lanes: every rank starts its
    lane children, the lane-l children of all ranks join a process group of their own (a TCP store on a port rank 0 hands out;
    under torch.distributed.run a tcp:// rendezvous would wait for the elastic agent's store: the first GPU rehearsal hung there),
    and every group does one all-reduce of (lane + 1): group l of N ranks must see N (l + 1)."""
    import json
    import os
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--rendezvous-only"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and json.loads(lines[0]) == {"n_gpus": 2, "rendezvous_only": True, "lanes": 2, "lane_group_sums": [2, 4]}, r.stdout
    r3 = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--lanes", "3", "--rendezvous-only"], env=env, capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0 and json.loads(r3.stdout.strip())["lane_group_sums"] == [2, 4, 6], r3.stderr[-2000:]
    bad = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "8", "--rendezvous-only"], env=dict(env, WORLD_SIZE="1", RANK="0"),
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "refusing" in bad.stderr and not bad.stdout.strip()
    one = subprocess.run([sys.executable, str(root / "bench.py"), "--rendezvous-only"], env=env, capture_output=True, text=True, timeout=120)
    assert one.returncode == 0 and json.loads(one.stdout.strip()) == {"n_gpus": 1, "rendezvous_only": True, "lanes": 2, "lane_group_sums": [1, 2]}


def test_bench_lanes_and_the_ordered_exchange():
    """Two ranks x two lanes hung in round 3: the lanes' host threads issued their steps' all-gathers in any order.  ``bench.py``
    now hands the exchanges of a multi-lane run to ``OrderedExchange`` -- one thread per rank that issues them in STEP order,
    whatever order the lanes finish in.  Checked here without a GPU-side collective: steps submitted out of order (by two
    threads) come out in order 0..n-1, each after its own event; an aborted run ends the thread."""
    import importlib.util
    import threading
    import time
    from pathlib import Path

    spec = importlib.util.spec_from_file_location("bench_mod", Path(__file__).resolve().parent.parent / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.resolve_lanes(2, 8, overlap=True, graph=True) == 2 and bench.resolve_lanes(9, 1, overlap=True, graph=True) == 4
    assert bench.resolve_lanes(2, 1, overlap=False, graph=True) == 1 and bench.resolve_lanes(2, 8, overlap=True, graph=False) == 1
    # the parity step is one that lane 0 (the rank process) runs over batch 0
    assert bench.parity_step_of(20, 2, 2, 0) == 18 and bench.parity_step_of(6, 2, 2, 0) == 4 and bench.parity_step_of(20, 2, 3, 0) == 18
    assert bench.parity_step_of(20, 2, 1, 0) == 18 and bench.parity_step_of(20, 1, 2, 0) == 18 and bench.parity_step_of(16, 16, 2, 256) == 0

    class FakeEvent:
        pass

    class FakeStream:
        def __init__(self, *a, **k):
            self.waited = []

        def wait_event(self, e):
            self.waited.append(e)

    class FakeCtx:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    order = []
    real = bench.torch.cuda
    fake_cuda = type("C", (), {"set_device": staticmethod(lambda i: None), "Stream": FakeStream, "stream": staticmethod(lambda s: FakeCtx())})
    bench.torch.cuda = fake_cuda
    try:
        n = 12
        ox = bench.OrderedExchange(0, n, lambda h, p: order.append((h, p)))

        def lane(idxs, delay):
            for i in idxs:
                time.sleep(delay)
                ox.submit(i, i, -i, FakeEvent())

        ths = [threading.Thread(target=lane, args=(list(range(1, n, 2)), 0.001)), threading.Thread(target=lane, args=(list(range(0, n, 2)), 0.004))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        ox.finish()
        assert order == [(i, -i) for i in range(n)]
        ox2 = bench.OrderedExchange(0, 5, lambda h, p: order.append("x"))
        ox2.submit(0, 0, 0, FakeEvent())
        time.sleep(0.05)
        ox2.finish(failed=True)                      # a lane died: the exchange thread must not wait for step 1 for ever
        assert not ox2.thread.is_alive()
    finally:
        bench.torch.cuda = real


def test_bench_dump_outputs_of_a_step(tmp_path):
    """``bench.py --dump-outputs``: one step's tile results as float32 / float64 arrays -- per instance score, class, tile and
    pixel count, per contour record the 12 measurements, and the row / column pixel counts of the masks -- within 64 MB; over
    that bound the profiles cover a fixed seeded sample of the instances."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", Path(__file__).resolve().parent.parent / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    size = 64
    res, dense, n_rec = [], [], 0
    for t in range(3):
        m, s, c = _make_unit(t, size, size)
        recs = []
        for i in range(len(s)):
            recs.append([{"values": np.arange(12.0) + 100 * (n_rec + k), "area": 7.0 + k, "perimeter": 3.5 + k} for k in range(i % 3)])
            n_rec += i % 3
        res.append((_pack(m) if len(m) else None, [np.float32(v) for v in s], list(c), recs))
        dense += list(m)
    dense = np.stack(dense)
    bench.dump_step_outputs(str(tmp_path / "a"), res, size)
    got = {f.stem: np.load(f) for f in (tmp_path / "a").glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    n = dense.shape[0]
    assert got["scores"].dtype == np.float32 and np.array_equal(got["scores"], np.concatenate([np.float32(r[1]) for r in res]))
    assert np.array_equal(got["classes"], np.concatenate([r[2] for r in res]).astype(np.float32))
    assert np.array_equal(got["tile"], np.concatenate([[t] * len(r[1]) for t, r in enumerate(res)]).astype(np.float32))
    assert np.array_equal(got["mask_area"], dense.sum((1, 2))) and np.array_equal(got["mask_sample"], np.arange(n, dtype=np.float32))
    assert np.array_equal(got["mask_row_pixels"], dense.sum(2)) and np.array_equal(got["mask_col_pixels"], dense.sum(1))
    assert got["measurements"].shape == (n_rec, 12) and np.array_equal(got["measurements"], 100.0 * np.arange(n_rec)[:, None] + np.arange(12.0))
    assert np.array_equal(got["measurement_instance"], [i for i, cs in enumerate(c_ for r in res for c_ in r[3]) for _ in cs])
    assert np.array_equal(got["contour_area"] - got["contour_perimeter"], np.full(n_rec, 3.5))
    # a bound that leaves room for two instances' profiles: a seeded sample of two, the rest of the arrays whole
    bench.DUMP_LIMIT_BYTES = sum(a.nbytes for k, a in got.items() if not k.startswith("mask_")) + 8 * n + 2 * (8 * size + 4)
    bench.dump_step_outputs(str(tmp_path / "b"), res, size)
    small = {f.stem: np.load(f) for f in (tmp_path / "b").glob("*.npy")}
    pick = small["mask_sample"].astype(np.int64)
    assert len(pick) == 2 and np.array_equal(small["mask_row_pixels"], dense[pick].sum(2)) and np.array_equal(small["mask_area"], got["mask_area"])
    assert sum(a.nbytes for a in small.values()) <= bench.DUMP_LIMIT_BYTES


def _worker_status(rank, world, port, h, w, out):
    """Three exchanges; in the second one rank 1 reports that its local share FAILED (empty table, status 1)."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deepemia_amd import parallel as PL

    state = PL.ExchangeState()
    log = []
    for step in range(3):
        failed = step == 1 and rank == 1
        mine = [] if failed else PL.shard_indices(6, rank, world)
        masks, scores, classes, units = [np.zeros((0, h, w), bool)], [], [], []
        for u in mine:
            m, s, c = _make_unit(10 * step + u, h, w)
            masks.append(m)
            scores += list(s)
            classes += list(c)
            units += [u] * len(s)
        masks = np.concatenate(masks)
        bb, area = _bbox_area(masks)
        hdr, pay = PL.encode_instance_table(_pack(masks) if len(masks) else None, scores, classes, units, bb, area)
        gt = PL.all_gather_instance_tables(hdr, pay, status=1 if failed else 0, state=state)
        packed, gs, gc, gu = PL.decode_instance_table(gt.header, gt.payload, h, w, host_header=gt.host_header, offsets=gt.offsets)
        log.append((gt.status.tolist(), packed.numpy(), gs, gc, gu))
    out[rank] = (log, dict(state.stats), dict(PL.stats))
    dist.barrier()
    dist.destroy_process_group()


def test_a_failed_rank_still_takes_part_and_every_rank_reads_the_same_status_words():
    """a rank whose share of an image failed used to skip the image's all-gather and meet its peers' NEXT
    all-gather with another image's tables.  Now the status travels in the slot: every rank sees [0, 1] for that exchange
    (and skips the image together), and the exchange after it is aligned and exact.  The capacities live in the caller's
    ``ExchangeState``: the module default is untouched."""
    h, w, world = 48, 96, 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_status, args=(world, _free_port(), h, w, out), nprocs=world, join=True)
    for r in range(world):
        log, st, default_stats = out[r]
        assert [x[0] for x in log] == [[0, 0], [0, 1], [0, 0]]
        assert st["exchanges"] == 3 and default_stats["exchanges"] == 0
    for step in (0, 2):                       # the good exchanges are exact and identical on both ranks
        em, es, ec, eu = [], [], [], []
        for u in range(6):
            m, s, c = _make_unit(10 * step + u, h, w)
            em.append(m)
            es += [float(v) for v in s]
            ec += [int(v) for v in c]
            eu += [u] * len(s)
        exp = _pack(np.concatenate(em)).numpy()
        for r in range(world):
            _, packed, gs, gc, gu = out[r][0][step]
            assert gu == eu and gc == ec and gs == es
            np.testing.assert_array_equal(packed, exp)


def _synthetic_table(rank, world, n, rng, interleaved):
    """A rank's table as the 48-tile bench step produces it: ~n instances with ~90-word cropped payloads (~1 MB)."""
    hdr = np.zeros((n, 10), dtype=np.int32)
    tile = np.sort(rng.integers(0, 48, n))
    hdr[:, 0] = tile * world + rank if interleaved else rank * 48 + tile       # unit i -> rank i % world, or blocked
    hdr[:, 1] = rng.integers(0, 2, n)
    hdr[:, 2:4] = rng.uniform(0.3, 1.0, n).reshape(n, 1).view(np.int32)
    y0, x0 = rng.integers(0, 1900, n), rng.integers(0, 1900, n)
    hh, ww = rng.integers(10, 120, n), rng.integers(10, 120, n)
    hdr[:, 4], hdr[:, 5], hdr[:, 6], hdr[:, 7] = y0, x0, y0 + hh, x0 + ww
    hdr[:, 8] = hh * ww // 2
    from deepemia_amd import parallel as PL
    total = int(PL._payload_lengths(hdr).sum())
    return hdr, rng.integers(-2**31, 2**31 - 1, total, dtype=np.int64).astype(np.int32)


def _worker_world8(rank, world, port, out):
    import time
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from deepemia_amd import parallel as PL

    res = {}
    for interleaved in (False, True):
        state = PL.ExchangeState()
        rng = np.random.default_rng(100 + rank)
        times, dec, mrg, rows, words = [], [], [], 0, 0
        for step in range(4):
            hdr, pay = _synthetic_table(rank, world, 2700 + 40 * rank, rng, interleaved)
            dist.barrier()
            t0 = time.perf_counter()
            gt = PL.all_gather_instance_tables(torch.from_numpy(hdr), torch.from_numpy(pay), state=state)
            t1 = time.perf_counter()
            # the decode's own CPU time: eight ranks share the cores, and a wall clock here also counts the slices the OS gives
            # the other ranks (a 2 ms decode can read 60-100 ms when the eight ranks have eight cores between them)
            c1 = time.thread_time()
            scores, classes, units, lens, _ = PL.decode_header(gt.host_header)
            offs = gt.offsets
            c2 = time.thread_time()
            times.append(t1 - t0)
            dec.append(c2 - c1)
            mrg.append(state.last_merge_ms)
            rows, words = int(gt.header.shape[0]), int(lens.sum())
            assert units == sorted(units) and len(scores) == rows == len(classes)
            # this rank's rows arrive intact: same payload words at the offsets the merged header says
            mine = np.nonzero((np.asarray(units) % world == rank) if interleaved else (np.asarray(units) // 48 == rank))[0]
            assert len(mine) == hdr.shape[0]
            np.testing.assert_array_equal(gt.host_header[mine], hdr)
            first = mine[0]
            np.testing.assert_array_equal(gt.payload.numpy()[offs[first]: offs[first] + lens[first]], pay[: lens[first]])
        res[interleaved] = dict(exchange_ms=[round(1e3 * t, 2) for t in times], decode_header_ms=[round(1e3 * t, 2) for t in dec],
                                merge_ms=[round(t, 2) for t in mrg], rows=rows, payload_mb=round(words * 4 / 1e6, 2), stats=dict(state.stats))
    out[rank] = res
    dist.barrier()
    dist.destroy_process_group()


def test_world8_exchange_of_realistic_tables_host_cost():
    """Eight ranks x ~2 800 instances x ~1 MB of cropped payload per step (the 48-tile bench step at N = 8), gloo on the CPU:
    the exchange is exact for blocked (bench) and interleaved (``i % world``, the CLI) unit ids, needs one host wait in
    the steady state, and its host-side cost -- the merge by unit id and the header decode, which RCCL does not make
    cheaper -- is printed and bounded (the payload permutation and the lists are numpy, no Python loop over instances)."""
    world = 8
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_world8, args=(world, _free_port(), out), nprocs=world, join=True)
    r0 = out[0]
    print("world-8 exchange, rank 0:", {("interleaved" if k else "blocked"): v for k, v in r0.items()})
    for inter in (False, True):
        v = r0[inter]
        assert v["rows"] == sum(2700 + 40 * r for r in range(world)) and v["payload_mb"] > 4.0
        assert v["stats"] == {"exchanges": 4, "size_exchanges": 1, "host_syncs": 5}
        # exchange_ms includes gloo's TCP all-gather of ~27 MB between eight processes sharing this container's cores (not
        # what RCCL will cost); the HOST work that stays at N = 8 is the merge by unit id (+ the payload permutation when
        # units interleave) and the header decode: both a few ms of numpy per 70 ms step
        assert max(v["merge_ms"][1:]) < 60.0, v
        assert max(v["decode_header_ms"]) < 30.0, v
