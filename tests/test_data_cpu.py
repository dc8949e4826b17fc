"""The host side of the device-resident dataset (pmoe_amd/data.py; runs without a GPU): the sample list and permutation of the
reference's CarlaSegPred, the measurement arithmetic, every refusal that comes before a device call, the argument checks of the
three gather entry points (csrc/dataset.hip), and the directory walk."""
import json
import math

import numpy as np
import pytest
import torch

from pmoe_amd import data, hip
from pmoe_amd.data import CarlaSeg, CarlaSegPred, FrameStore, SequenceIndex, measurement_table

LENGTHS = [13, 10, 9, 25, 3]


def _windows(lengths, past, future):
    """model/data_loader.py:175-196 written out over frame ids: (frames, measurement, masks) per sample, per episode count"""
    out, counts, base = [], [], 0
    for L in lengths:
        files = list(range(base, base + L))
        k = 0
        for i in range(len(files) - (past + future)):
            out.append((files[i:i + past], files[i + past] if i + past < len(files) else None, files[i + past:i + past + future]))
            k += 1
        counts.append(k)
        base += L
    return out, counts


@pytest.mark.parametrize("future,counts", [(6, [3, 0, 0, 15, 0]), (0, [9, 6, 5, 21, 0])])
def test_windows_are_the_reference_sample_list(future, counts):
    want, got_counts = _windows(LENGTHS, 4, future)
    assert got_counts == counts
    ix = SequenceIndex(LENGTHS, 4, future, seed=3)
    assert len(ix) == sum(counts) == len(want)
    assert ix.frames.dtype == ix.measurement.dtype == ix.masks.dtype == torch.int64
    assert ix.frames.tolist() == [w[0] for w in want]
    assert ix.measurement.tolist() == [w[1] for w in want]
    assert ix.masks.tolist() == [w[2] for w in want]
    assert tuple(ix.masks.shape) == (len(want), future)


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_indices_are_the_global_seed_permutation(seed):
    ix = SequenceIndex(LENGTHS, 4, 6, seed=seed)
    state = torch.random.get_rng_state()
    try:
        torch.random.manual_seed(seed)
        want = torch.randperm(len(ix))
    finally:
        torch.random.set_rng_state(state)
    assert torch.equal(ix.indices, want)
    before = torch.random.get_rng_state()
    SequenceIndex(LENGTHS, 4, 6, seed=seed)
    assert torch.equal(torch.random.get_rng_state(), before)            # the global generator is not touched


def _reference_measurements(m, speed_factor, n_commands):
    """data_loader.py:216-243 (_preprocess_measurements), statement by statement"""
    steer, brake, throttle = m["steer"], m["brake"], m["throttle"]
    speed = torch.tensor(m["speed"] / speed_factor, dtype=torch.float)
    target_speed = torch.tensor(m["target_speed"] / speed_factor, dtype=torch.float)
    command = torch.zeros(n_commands).scatter_(dim=0, index=torch.tensor(m["command"] - 1, dtype=torch.long), value=1)
    pedal = -brake if brake > 0.05 else throttle
    control = torch.tensor([steer, pedal], dtype=torch.float)
    return torch.cat([control, speed.reshape(1), target_speed.reshape(1), command])


def _records(n_commands, speed_factor):
    rng = np.random.default_rng(7)
    speeds = rng.uniform(0.0, 40.0, 4000)
    # speeds whose division differs in the last bit when it is done in f32 instead of double-then-round
    f32 = (speeds.astype(np.float32) / np.float32(speed_factor)).astype(np.float32)
    differs = speeds[f32 != (speeds / speed_factor).astype(np.float32)]
    assert len(differs) > 100
    recs = []
    brakes = [0.0, 0.05, math.nextafter(0.05, 1.0), 0.049999, 0.3, 1.0]
    for k in range(48):
        recs.append(dict(steer=float(rng.uniform(-1, 1)), brake=brakes[k % len(brakes)], throttle=float(rng.uniform(0, 1)),
                         speed=float(differs[k]), target_speed=float(differs[100 - k]), command=1 + k % n_commands))
    return recs


@pytest.mark.parametrize("n_commands,speed_factor", [(4, 10), (6, 12), (4, 3.6)])
def test_measurement_table_is_the_reference_arithmetic(n_commands, speed_factor):
    recs = _records(n_commands, speed_factor)
    assert {r["command"] for r in recs} == set(range(1, n_commands + 1))
    table = measurement_table(recs, speed_factor, n_commands)
    assert table.dtype == torch.float32 and tuple(table.shape) == (len(recs), 4 + n_commands)
    want = torch.stack([_reference_measurements(r, speed_factor, n_commands) for r in recs])
    assert torch.equal(table, want)
    # brake exactly 0.05 keeps the throttle; the next double above it brakes
    assert table[1, 1] == torch.tensor(recs[1]["throttle"], dtype=torch.float)
    assert table[2, 1] == -torch.tensor(recs[2]["brake"], dtype=torch.float)
    for bad in (0, n_commands + 1):
        with pytest.raises(ValueError, match="command"):
            measurement_table([dict(recs[0], command=bad)], speed_factor, n_commands)


# ---- refusals that come before any device call (this file runs on a machine without a GPU: a device call would raise something else)
def test_store_refuses_on_the_host():
    with pytest.raises(RuntimeError, match="no CPU path"):
        FrameStore(4, (1, 1), (8, 8), device="cpu")
    store = FrameStore(2, crop=(2, 1), size=(8, 8))
    ok = torch.zeros(1, 12, 16, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        store.append(ok.float())
    with pytest.raises(TypeError, match="uint8"):
        store.append(np.zeros((1, 12, 16, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="channel"):
        store.append(torch.zeros(1, 12, 16, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="capacity"):
        store.append(torch.zeros(3, 12, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no rows"):
        store.append(torch.zeros(1, 3, 16, 3, dtype=torch.uint8))
    store.raw_size = (12, 16)                                           # (as after a first append)
    with pytest.raises(ValueError, match="12 x 16"):
        store.append(torch.zeros(1, 12, 20, 3, dtype=torch.uint8))
    store.count = 2
    with pytest.raises(ValueError, match="capacity"):
        store.append(ok)
    masks = FrameStore(2, crop=(2, 1), size=(8, 8), channels=1)
    with pytest.raises(ValueError, match="channel"):
        masks.append(torch.zeros(1, 12, 16, 3, dtype=torch.uint8))
    assert store.data is None and masks.data is None                    # nothing was allocated


def test_dataset_refuses_on_the_host():
    frames = np.zeros((8, 12, 16, 3), dtype=np.uint8)
    for cls, kw in ((CarlaSegPred, dict(past_frames=2, future_frames=1)), (CarlaSeg, {})):
        with pytest.raises(ValueError, match="'train' or 'val'"):
            cls.from_arrays([dict(rgb=frames, mask=frames[..., 0])], mode="test", **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            cls.from_arrays([dict(rgb=frames, mask=frames[..., 0])], mode="val", device="cpu", **kw)
    with pytest.raises(ValueError, match="Unknown augmentation"):
        CarlaSegPred.from_arrays([dict(rgb=frames, mask=frames[..., 0])], aug_type="nope")
    with pytest.raises(ValueError, match="8 frames and 7 mask"):
        CarlaSegPred.from_arrays([dict(rgb=frames, mask=frames[:7, ..., 0])], 2, 1, mode="val")
    # sample ids are checked against the sample list, on the host
    ds = CarlaSegPred.__new__(CarlaSegPred)
    ds._setup(4, 2, "segmentation", "val", 0, False, 32, 1, (2, 1), (8, 8), 10, 4, "cuda")
    ds._make_stores(25)
    ds._finish([13, 12], None)
    assert len(ds) == 13
    for bad in ([13], [-1], [0, 99], []):
        with pytest.raises((IndexError, ValueError), match="sample ids"):
            ds.batch(bad)
    with pytest.raises(ValueError, match="world"):
        ds.loader(5, rank=2, world=2)
    assert len(ds.loader(5)) == 3 and len(ds.loader(5, drop_last=True, num_workers=8, pin_memory=True, worker_init_fn=None)) == 2


# ---- the library
NAMES = ("pmoe_gather_rows", "pmoe_gather_frames_to_f32", "pmoe_gather_labels_to_i64")
p1, p2, p3 = 0x1000, 0x2000, 0x3000                                     # 16-byte aligned, never dereferenced
# entry point -> (accepted arguments, [{argument index: value that is refused}, ...]), in the style of tests/entry_refusals.py
REFUSALS = {
    "pmoe_gather_rows": ([p1, p2, p3, 37, 5, 3072, None],
                         [{0: None}, {1: None}, {2: None}, {3: 0}, {3: -1}, {4: 0}, {4: -2}, {5: 0}, {5: -16}, {2: p1}]),
    "pmoe_gather_frames_to_f32": ([p1, p2, p3, 37, 5, 32, 32, 3, None],
                                  [{0: None}, {1: None}, {2: None}, {3: 0}, {4: 0}, {4: -1}, {5: 0}, {6: 0}, {6: -3}, {7: 0},
                                   {5: 32768, 6: 16384}]),
    "pmoe_gather_labels_to_i64": ([p1, p2, p3, 37, 5, 1024, None],
                                  [{0: None}, {1: None}, {2: None}, {3: 0}, {4: 0}, {5: 0}, {5: -4}]),
}


def test_library_exports_the_gathers():
    lib = hip.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert set(REFUSALS) == set(NAMES)
    assert lib.pmoe_version() == 401


# (with a GPU, a check that got lost would launch a kernel on the made-up pointers below)
@pytest.mark.skipif(torch.cuda.is_available(), reason="a lost check would launch on made-up device pointers")
def test_gather_entry_points_refuse_bad_arguments():
    lib = hip.load()
    for name, (good, changes) in REFUSALS.items():
        for change in changes:
            args = list(good)
            for i, v in change.items():
                args[i] = v
            assert getattr(lib, name)(*args) == hip.ERR_ARG, (name, change)
        # the accepted list passes every check: without a GPU the launch behind them fails in the runtime (a HIP error > 0)
        assert getattr(lib, name)(*good) > 0, name
    # unaligned bases and odd row sizes are served (the 4-byte and byte paths), not refused
    for src, dst, row in ((p1 + 4, p3, 108), (p1 + 1, p3, 3072), (p1, p3 + 2, 105)):
        assert lib.pmoe_gather_rows(src, p2, dst, 37, 5, row, None) > 0


# ---- directory ingest
class _RecordingStore:
    """stands in for a FrameStore: keeps what append is given"""

    def __init__(self, *a, **k):
        self.got, self.device, self.count = [], torch.device("cuda"), 0

    def append(self, frames):
        assert isinstance(frames, np.ndarray) and frames.dtype == np.uint8
        self.got.append(frames.copy())
        self.count += len(frames)

    def release_staging(self):
        pass

    def all(self):
        return np.concatenate(self.got)


def _write_tree(root, episodes):
    from PIL import Image
    for name, (rgb, mask, meas) in episodes.items():
        for sub in ("rgb", "mask", "measurements"):
            (root / name / sub).mkdir(parents=True)
        for i in reversed(range(len(rgb))):                             # (written out of order: the walk sorts)
            Image.fromarray(rgb[i]).save(root / name / "rgb" / f"{i:04d}.png")
            Image.fromarray(mask[i]).save(root / name / "mask" / f"{i:04d}.png")
            (root / name / "measurements" / f"{i:04d}.json").write_text(json.dumps(meas[i]))
        (root / name / "rgb" / "notes.txt").write_text("not a frame")
    (root / "README.txt").write_text("not an episode")


def _episode(rng, n, first):
    rgb = rng.integers(0, 256, (n, 24, 32, 3), dtype=np.uint8)
    mask = rng.integers(0, 23, (n, 24, 32), dtype=np.uint8)
    meas = [dict(steer=0.1 * k, brake=0.0, throttle=0.5, speed=float(first + k), target_speed=7.0, command=1 + k % 4) for k in range(n)]
    return rgb, mask, meas


def test_directory_ingest_walks_in_sorted_order(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    eps = {"town02_b": _episode(rng, 5, 100), "town01_a": _episode(rng, 7, 0)}   # (created in the other order)
    _write_tree(tmp_path, eps)
    order = ["town01_a", "town02_b"]
    rgb, mask = _RecordingStore(), _RecordingStore()
    lengths, records = data.ingest_directory(tmp_path, rgb, mask, measurements=True, threads=3)
    assert lengths == [7, 5]                                            # episode boundaries, in sorted order
    assert np.array_equal(rgb.all(), np.concatenate([eps[k][0] for k in order]))     # the decoded bytes reach append
    assert np.array_equal(mask.all(), np.concatenate([eps[k][1] for k in order]))
    assert records == [m for k in order for m in eps[k][2]]
    assert len(rgb.got) == 2                                            # chunk by chunk: no chunk spans two episodes
    # without masks / measurements those folders are not read
    rgb2 = _RecordingStore()
    assert data.ingest_directory(tmp_path, rgb2) == ([7, 5], None)
    # CarlaSeg's form: one list over all episodes, sorted by full path
    rgb3, mask3 = _RecordingStore(), _RecordingStore()
    assert data.ingest_directory(tmp_path, rgb3, mask3, flat=True)[0] == [12]
    assert np.array_equal(rgb3.all(), rgb.all()) and np.array_equal(mask3.all(), mask.all())
    # the datasets over the same tree (the stores stubbed out: no device)
    monkeypatch.setattr(data, "FrameStore", _RecordingStore)
    ds = CarlaSegPred(str(tmp_path), past_frames=2, future_frames=1, mode="val", crop=(2, 1), resize=(8, 8))
    assert len(ds) == (7 - 3) + (5 - 3) and ds.index.episode_lengths == [7, 5]
    assert np.array_equal(ds.store.all(), rgb.all()) and np.array_equal(ds.mask_store.all(), mask.all())
    seg = CarlaSeg(str(tmp_path), mode="val", crop=(2, 1), resize=(8, 8))
    assert len(seg) == 12 and seg.index.frames.reshape(-1).tolist() == list(range(12))
    # a mask that is not single-channel is refused; so is an episode whose folders disagree
    from PIL import Image
    Image.fromarray(eps["town01_a"][0][0]).save(tmp_path / "town01_a" / "mask" / "0003.png")
    with pytest.raises(ValueError, match="single-channel"):
        data.ingest_directory(tmp_path, _RecordingStore(), _RecordingStore())
    (tmp_path / "town02_b" / "mask" / "0004.png").unlink()
    with pytest.raises(ValueError, match="5 rgb frames and 4 mask"):
        data.ingest_directory(tmp_path, _RecordingStore(), _RecordingStore())


def test_ingest_threads_come_from_the_cpu_share():
    assert 1 <= data.cpu_share() <= data.MAX_INGEST_THREADS == 16
    assert data.cpu_share(cap=2) <= 2
