"""Device-resident dataset: the reference's ``CarlaSeg`` / ``CarlaSegPred`` (``model/data_loader.py``) with the pixels kept in HBM.

``Crop -> Resize`` is a pure function of a frame and everything random (the augmenter) comes after it
(``data_loader.py:255-271``), so the resized uint8 frame is computed once at ingest (``FramePreprocessor.resized``) and kept in a
``FrameStore`` (150,528 bytes per 224 x 224 RGB frame).  A batch is then an int64 index table, built and checked on the host and
sent up in one pinned non-blocking copy, plus one gather (``csrc/dataset.hip``) -- no host-side pixel work per step, no
host-to-device pixel traffic, and the T - 1 frames that consecutive windows share are resized once, not T times.

What is the reference's: the constructor arguments, the sample list (``SequenceIndex``), ``indices`` (the seeded ``randperm``), the
measurement arithmetic (``measurement_table``), the tensors a ``DataLoader`` over the dataset yields.  What is not claimed: the
stream of ``DataLoader``'s sampler (``loader`` shuffles with ``torch.randperm``), imgaug's bits (``pmoe_amd/augment.py`` says what
the augmenter does claim), and the reference's per-SAMPLE augmenter schedule: the reference rebuilds ``get_augmenter(boost * k)`` for
the k-th sample a worker process reads (so its counter also depends on ``num_workers``); here the augmenter is built once per
BATCH from ``boost * samples_read_so_far``.  Inside a batch the schedule factors of the two differ by about 1e-5.

There is no CPU path: a store lives on the MI355X, and a missing kernel is an error.
"""
import ctypes as C
import json
import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import torch

from .augment import get_augmenter, run_plan
from .hip import check, load, stream_ptr
from .parallel import shard_batch
from .preprocess import FramePreprocessor

MAX_INGEST_THREADS = 16
INGEST_CHUNK = 64                              # frames per upload / resize call (92 MB of raw 600 x 800 RGB)


def _p(t):
    return C.c_void_p(t.data_ptr())


def cpu_share(cap=MAX_INGEST_THREADS):
    """CPUs this process may use, at most ``cap``: the cgroup quota where there is one, else the affinity mask -- never
    ``os.cpu_count()``, which shows the whole machine."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = 1
    try:
        quota, period = Path("/sys/fs/cgroup/cpu.max").read_text().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return max(1, min(n, int(cap)))


# ---------------------------------------------------------------------------------------------------------------- the gathers
def _gather_args(store, idx, who, dtype):
    for t, name in ((store, "store"), (idx, "idx")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a tensor on the MI355X (cuda) device; pmoe_amd has no CPU path")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
    if dtype is not None and store.dtype != dtype:
        raise ValueError(f"{who}: expected a {dtype} store, got {store.dtype}")
    if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() < 1 or idx.device != store.device:
        raise ValueError(f"{who}: idx must be a non-empty int64 vector on the store's device")
    if store.dim() < 2 or store.shape[0] < 1 or store[0].numel() < 1:
        raise ValueError(f"{who}: expected a store of at least one non-empty row")


def gather_rows(store, idx, n_src=None):
    """``store[idx]`` for a dense device tensor ``[N, ...]`` of any dtype and an int64 device vector ``idx`` (values in
    ``[0, n_src)``, ``n_src`` = the rows in use, default ``N``; a row outside it comes back as zeros): ``pmoe_gather_rows``."""
    _gather_args(store, idx, "gather_rows", None)
    n = idx.numel()
    out = torch.empty((n,) + tuple(store.shape[1:]), dtype=store.dtype, device=store.device)
    with torch.cuda.device(store.device):
        check(load().pmoe_gather_rows(_p(store), _p(idx), _p(out), store.shape[0] if n_src is None else int(n_src), n,
                                      store[0].numel() * store.element_size(), stream_ptr()), "pmoe_gather_rows")
    return out


def gather_frames_to_f32(store, idx, n_src=None):
    """uint8 ``[N, h, w, C]`` -> float32 ``[n, C, h, w]`` = ``store[idx].permute(0, 3, 1, 2) / 255`` (ToTensor), one launch"""
    _gather_args(store, idx, "gather_frames_to_f32", torch.uint8)
    if store.dim() != 4:
        raise ValueError("gather_frames_to_f32: expected a store [N, h, w, C]")
    n, (_, h, w, c) = idx.numel(), store.shape
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=store.device)
    with torch.cuda.device(store.device):
        check(load().pmoe_gather_frames_to_f32(_p(store), _p(idx), _p(out), store.shape[0] if n_src is None else int(n_src), n,
                                               h, w, c, stream_ptr()), "pmoe_gather_frames_to_f32")
    return out


def gather_labels_to_i64(store, idx, n_src=None):
    """uint8 ``[N, ...]`` -> int64 ``[n, ...]`` = ``store[idx].long()`` (MaskPILToTensor), one launch"""
    _gather_args(store, idx, "gather_labels_to_i64", torch.uint8)
    n = idx.numel()
    out = torch.empty((n,) + tuple(store.shape[1:]), dtype=torch.int64, device=store.device)
    with torch.cuda.device(store.device):
        check(load().pmoe_gather_labels_to_i64(_p(store), _p(idx), _p(out), store.shape[0] if n_src is None else int(n_src), n,
                                               store[0].numel(), stream_ptr()), "pmoe_gather_labels_to_i64")
    return out


# ---------------------------------------------------------------------------------------------------------------- frame store
class FrameStore:
    """uint8 ``[capacity, h, w, channels]`` on the device: the Resize output of every frame appended so far.

    ``append(frames)`` takes raw uint8 frames ``[n, H0, W0, channels]`` (one frame: ``[H0, W0, channels]``; with ``channels=1``
    class-id images ``[n, H0, W0]``), as a device tensor (used directly), a CPU tensor or a numpy array (sent up in pinned chunks),
    runs ``Crop -> Resize`` on the device, writes the next slots and returns their ids as a ``range``.  Everything that can be
    refused -- dtype, channel count, a frame size other than the first append's, a crop that leaves no rows, overflow, a tensor on
    another device -- is refused before any launch.  The device memory is allocated at the first append."""

    def __init__(self, capacity, crop=(125, 90), size=(224, 224), channels=3, device="cuda"):
        self.capacity, self.channels = int(capacity), int(channels)
        if self.capacity < 1 or self.channels < 1:
            raise ValueError("FrameStore: capacity and channels must be at least 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"FrameStore: the store lives on the MI355X (cuda) device, got {self.device}; pmoe_amd has no CPU path")
        self.pre = FramePreprocessor(crop, size)
        self.h, self.w = self.pre.size
        self.count = 0
        self.raw_size = None                    # (H0, W0) of the first append
        self.data = None
        self._pin, self._events = [None, None], [None, None]

    def __len__(self):
        return self.count

    @property
    def row_bytes(self):
        return self.h * self.w * self.channels

    def _checked(self, frames):
        """-> uint8 tensor [n, H0, W0, channels] (a view where possible); raises before anything touches the device"""
        if not isinstance(frames, torch.Tensor):
            import numpy as np
            if not isinstance(frames, np.ndarray):
                raise TypeError("FrameStore.append: expected a torch tensor or a numpy array")
            if frames.dtype != np.uint8:
                raise TypeError(f"FrameStore.append: expected uint8 frames, got {frames.dtype}")
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dtype != torch.uint8:
            raise TypeError(f"FrameStore.append: expected uint8 frames, got {frames.dtype}")
        if frames.is_cuda and frames.device != self._resolved_device():
            raise RuntimeError(f"FrameStore.append: frames are on {frames.device}, the store is on {self.device}")
        t = frames
        if self.channels == 1 and t.dim() == 3:
            t = t.unsqueeze(-1)                 # [n, H0, W0] class-id images
        elif t.dim() == 3:
            t = t.unsqueeze(0)                  # one frame [H0, W0, C]
        if t.dim() != 4:
            raise ValueError(f"FrameStore.append: expected [n, H0, W0, {self.channels}], got {tuple(frames.shape)}")
        n, H0, W0, ch = t.shape
        if ch != self.channels:
            raise ValueError(f"FrameStore.append: the store holds {self.channels}-channel frames, got {ch} channels")
        if self.raw_size is not None and (H0, W0) != self.raw_size:
            raise ValueError(f"FrameStore.append: frames of {H0} x {W0}, the store was filled from {self.raw_size[0]} x {self.raw_size[1]}")
        if H0 - self.pre.top - self.pre.bottom < 1 or W0 < 1:
            raise ValueError(f"FrameStore.append: crop ({self.pre.top}, {self.pre.bottom}) leaves no rows of a {H0}-row frame")
        if self.count + n > self.capacity:
            raise ValueError(f"FrameStore.append: {n} frames after {self.count} exceed the capacity of {self.capacity}")
        return t

    def _resolved_device(self):
        """the store's device with its index filled in (``cuda`` means the current device) -- no device call unless needed"""
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def append(self, frames):
        t = self._checked(frames)
        n = t.shape[0]
        first = self.count
        if n:
            self._write(t)
            self.raw_size = (int(t.shape[1]), int(t.shape[2]))
            self.count = first + n
        return range(first, first + n)

    def _write(self, t):
        """the device side of ``append``: upload (CPU frames), Crop -> Resize, the next slots"""
        with torch.cuda.device(self.device):
            if self.data is None:
                self.data = torch.empty(self.capacity, self.h, self.w, self.channels, dtype=torch.uint8, device=self.device)
            for k, a in enumerate(range(0, t.shape[0], INGEST_CHUNK)):
                part = t[a:a + INGEST_CHUNK]
                src = part if part.is_cuda else self._upload(part, k & 1)
                dst = self.data[self.count + a:self.count + a + part.shape[0]]
                dst.copy_(self.pre.resized(src))

    def _upload(self, part, slot):
        """CPU frames -> device through one of two pinned buffers (the event says when a buffer's last copy has left it)"""
        buf, ev = self._pin[slot], self._events[slot]
        if buf is None or buf.shape[0] < part.shape[0] or buf.shape[1:] != part.shape[1:]:
            buf = self._pin[slot] = torch.empty((INGEST_CHUNK,) + tuple(part.shape[1:]), dtype=torch.uint8, pin_memory=True)
        elif ev is not None:
            ev.synchronize()
        buf[:part.shape[0]].copy_(part)
        dev = buf[:part.shape[0]].to(self.device, non_blocking=True)
        ev = self._events[slot] = torch.cuda.Event()
        ev.record()
        return dev

    def release_staging(self):
        """drop the pinned upload buffers (after the last append)"""
        for ev in self._events:
            if ev is not None:
                ev.synchronize()
        self._pin, self._events = [None, None], [None, None]


# ---------------------------------------------------------------------------------------------------------------- sample list
class SequenceIndex:
    """The sample list of ``CarlaSegPred.__init__`` (``data_loader.py:173-199``) over frame ids: episode e of ``L`` frames owns the
    ids ``base_e .. base_e + L - 1`` (episodes in the order given) and yields ``L - (past + future)`` windows -- the reference's
    ``range(len - seq_len)`` drops the last possible window, and so does this.  Window i of an episode: ``frames`` ids
    ``i .. i + past - 1``, ``measurement`` the id ``i + past``, ``masks`` ids ``i + past .. i + past + future - 1``.

    ``frames [n, past]``, ``measurement [n]``, ``masks [n, future]`` are int64 CPU tensors; ``indices`` is
    ``torch.randperm(n, generator=torch.Generator().manual_seed(seed))`` -- the permutation the reference draws with
    ``torch.random.manual_seed(seed); torch.randperm(n)``, without touching the global generator."""

    def __init__(self, episode_lengths, past_frames=4, future_frames=6, seed=0):
        self.past, self.future = int(past_frames), int(future_frames)
        if self.past < 1 or self.future < 0:
            raise ValueError("SequenceIndex: past_frames >= 1 and future_frames >= 0")
        self.episode_lengths = [int(L) for L in episode_lengths]
        if any(L < 0 for L in self.episode_lengths):
            raise ValueError("SequenceIndex: negative episode length")
        seq = self.past + self.future
        starts, base = [], 0
        for L in self.episode_lengths:
            starts.extend(range(base, base + max(L - seq, 0)))
            base += L
        self.n_frames = base
        first = torch.tensor(starts, dtype=torch.int64)
        self.frames = first[:, None] + torch.arange(self.past, dtype=torch.int64)[None, :]
        self.measurement = first + self.past
        self.masks = first[:, None] + self.past + torch.arange(self.future, dtype=torch.int64)[None, :]
        self.indices = torch.randperm(len(starts), generator=torch.Generator().manual_seed(int(seed)))

    def __len__(self):
        return int(self.frames.shape[0])


def measurement_table(records, speed_factor=10, n_commands=4):
    """One f32 row per frame from its measurement record (a dict with ``steer``, ``brake``, ``throttle``, ``speed``,
    ``target_speed``, ``command``): ``[steer, pedal, speed / speed_factor, target_speed / speed_factor, one-hot(command - 1)]``,
    ``pedal = -brake if brake > 0.05 else throttle`` -- ``_preprocess_measurements`` (``data_loader.py:216-243``) exactly: the
    divisions are Python doubles rounded to f32 once (dividing in f32 differs in the last bit for more than a quarter of random
    speeds).  A command outside ``1 .. n_commands`` raises ``ValueError`` (the reference's ``scatter_`` fails on it).
    -> CPU float32 ``[len(records), 4 + n_commands]``."""
    n_commands = int(n_commands)
    rows = []
    for i, m in enumerate(records):
        brake = m["brake"]
        pedal = -brake if brake > 0.05 else m["throttle"]
        command = m["command"]
        if int(command) != command or not 1 <= int(command) <= n_commands:
            raise ValueError(f"measurement_table: record {i} has command {command!r}, expected 1..{n_commands}")
        onehot = [0.0] * n_commands
        onehot[int(command) - 1] = 1.0
        rows.append([float(m["steer"]), float(pedal), m["speed"] / speed_factor, m["target_speed"] / speed_factor] + onehot)
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32).reshape(len(rows), 4 + n_commands)


# ---------------------------------------------------------------------------------------------------------------- directory ingest
def _decode_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "RGB":
            raise ValueError(f"{path}: expected an 8-bit RGB image, got mode {im.mode}")
        import numpy as np
        return np.asarray(im)


def _decode_mask(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "L":
            raise ValueError(f"{path}: a mask is a single-channel 8-bit image, got mode {im.mode}")
        import numpy as np
        return np.asarray(im)


def _files(folder, suffix):
    return sorted(str(x) for x in Path(folder).iterdir() if x.suffix == suffix)


def _append_decoded(pool, decode, paths, store):
    import numpy as np
    for a in range(0, len(paths), INGEST_CHUNK):
        store.append(np.stack(list(pool.map(decode, paths[a:a + INGEST_CHUNK]))))


def ingest_directory(root, rgb_store, mask_store=None, measurements=False, flat=False, threads=None):
    """Walk ``root/<episode>/{rgb,mask,measurements}`` like the reference: the ``.png`` / ``.json`` files of each folder in sorted
    order, the episodes in sorted order (``flat``: ``CarlaSeg``'s form, all frames of all episodes sorted by their full path, one
    episode).  PNGs are decoded with PIL in a pool of at most 16 threads (``cpu_share``) and appended to the stores chunk by
    chunk: ``rgb/`` to ``rgb_store``; ``mask/`` to ``mask_store`` when there is one.  -> (episode lengths, measurement records or
    None).  An episode whose folders disagree in length is refused."""
    root = Path(root).resolve()
    dirs = sorted(x for x in root.iterdir() if x.is_dir())
    episodes = []                               # (rgb paths, mask paths, measurement paths)
    for d in dirs:
        episodes.append((_files(d / "rgb", ".png"), _files(d / "mask", ".png") if mask_store is not None else None,
                         _files(d / "measurements", ".json") if measurements else None))
    if flat and episodes:
        merged = [None if episodes[0][k] is None else sorted(p for e in episodes for p in e[k]) for k in range(3)]
        episodes = [tuple(merged)]
    for rgb, mask, meas in episodes:
        for other, what in ((mask, "mask"), (meas, "measurements")):
            if other is not None and len(other) != len(rgb):
                raise ValueError(f"ingest_directory: {len(rgb)} rgb frames and {len(other)} {what} files in one episode of {root}")
    records = [] if measurements else None
    with ThreadPoolExecutor(max_workers=cpu_share() if threads is None else max(1, min(int(threads), MAX_INGEST_THREADS))) as pool:
        for rgb, mask, meas in episodes:
            _append_decoded(pool, _decode_rgb, rgb, rgb_store)
            if mask is not None:
                _append_decoded(pool, _decode_mask, mask, mask_store)
            if meas is not None:
                for path in meas:
                    with open(path, "r") as f:
                        records.append(json.load(f))
    return [len(e[0]) for e in episodes], records


def _count_frames(root):
    root = Path(root).resolve()
    return sum(len(_files(d / "rgb", ".png")) for d in root.iterdir() if d.is_dir())


# ---------------------------------------------------------------------------------------------------------------- datasets
class _Loader:
    """what ``DataLoader(dataset, batch_size, shuffle, drop_last)`` is to a training loop: an iterable of batches with a length"""

    def __init__(self, ds, batch_size, shuffle, drop_last, generator, rank, world):
        self.ds, self.batch_size, self.shuffle, self.drop_last = ds, int(batch_size), bool(shuffle), bool(drop_last)
        self.generator, self.rank, self.world = generator, int(rank), int(world)
        if self.batch_size < 1:
            raise ValueError("loader: batch_size must be at least 1")
        if not 0 <= self.rank < self.world:
            raise ValueError(f"loader: rank {rank} of world {world}")

    def __len__(self):
        n = len(self.ds)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.ds)
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        for k in range(len(self)):
            ids = order[k * self.batch_size:(k + 1) * self.batch_size]
            lo, hi = shard_batch(len(ids), self.rank, self.world)
            yield self.ds.batch(ids[lo:hi], generator=self.generator)


class CarlaSegPred:
    """``CarlaSegPred(root, past_frames, future_frames, aug_type, mode, seed, load_measurements, batch_size, boost, crop, resize,
    speed_factor, n_commands)`` of the reference with its frames resident on the device; ``from_arrays`` builds one from
    in-memory episodes.  ``len(ds)`` is the sample count, ``ds.indices`` the reference's permutation: sample ``i`` is window
    ``indices[i]`` of ``ds.index``.

    ``ds.loader(batch_size, shuffle, ...)`` yields what ``DataLoader(CarlaSegPred(...))`` yields, already on the device: ``img``
    f32 ``[B, T, 3, h, w]`` and, with ``load_measurements``, a dict of ``control [B, 2]``, ``speed [B]``, ``target_speed [B]``,
    ``command [B, n_commands]``, otherwise masks int64 ``[B, F, h, w]``."""

    _single = False                             # CarlaSeg: one frame and one mask per sample, no time axis

    def __init__(self, root="../data/train", past_frames=4, future_frames=6, aug_type="segmentation", mode="train", seed=0,
                 load_measurements=False, batch_size=32, boost=1, crop=(125, 90), resize=(224, 224), speed_factor=10,
                 n_commands=4, device="cuda"):
        self._setup(past_frames, future_frames, aug_type, mode, seed, load_measurements, batch_size, boost, crop, resize,
                    speed_factor, n_commands, device)
        self._make_stores(_count_frames(root))
        lengths, records = ingest_directory(root, self.store, self.mask_store, measurements=self.load_measurements,
                                            flat=self._single)
        self._finish(lengths, records)

    @classmethod
    def from_arrays(cls, episodes, past_frames=4, future_frames=6, aug_type="segmentation", mode="train", seed=0,
                    load_measurements=False, batch_size=32, boost=1, crop=(125, 90), resize=(224, 224), speed_factor=10,
                    n_commands=4, device="cuda"):
        """``episodes``: a list of dicts, each with ``rgb`` (uint8 ``[L, H0, W0, 3]``: numpy, CPU or device tensor) and either
        ``measurements`` (a list of ``L`` records, ``load_measurements=True``) or ``mask`` (uint8 ``[L, H0, W0]``)."""
        self = cls.__new__(cls)
        self._setup(past_frames, future_frames, aug_type, mode, seed, load_measurements, batch_size, boost, crop, resize,
                    speed_factor, n_commands, device)
        want = "measurements" if self.load_measurements else "mask"
        for e in episodes:
            if len(e[want]) != len(e["rgb"]):
                raise ValueError(f"from_arrays: an episode has {len(e['rgb'])} frames and {len(e[want])} {want} entries")
        self._make_stores(sum(len(e["rgb"]) for e in episodes))
        records = [] if self.load_measurements else None
        for e in episodes:
            self.store.append(e["rgb"])
            if self.load_measurements:
                records.extend(e["measurements"])
            else:
                self.mask_store.append(e["mask"])
        self._finish([len(e["rgb"]) for e in episodes], records)
        return self

    # ---- construction
    def _setup(self, past_frames, future_frames, aug_type, mode, seed, load_measurements, batch_size, boost, crop, resize,
               speed_factor, n_commands, device):
        if str(mode).lower() not in ("train", "val"):
            raise ValueError("Unknown parameter for mode, it should be 'train' or 'val'")
        self.mode = str(mode).lower()
        self.past_frames, self.future_frames = int(past_frames), int(future_frames)
        self.aug_type, self.seed, self.load_measurements = aug_type, int(seed), bool(load_measurements)
        self.batch_size, self.boost = int(batch_size), boost
        self.crop, self.resize = tuple(crop), tuple(resize)
        self.speed_factor, self.n_commands = speed_factor, int(n_commands)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: the dataset lives on the MI355X (cuda) device, got {self.device}; pmoe_amd has no CPU path")
        get_augmenter(1, self.batch_size, self.aug_type)        # an unknown aug_type is refused here, in either mode
        self.samples_read = 0

    def _make_stores(self, n_frames):
        cap = max(1, int(n_frames))
        self.store = FrameStore(cap, self.crop, self.resize, 3, self.device)
        self.mask_store = None if self.load_measurements else FrameStore(cap, self.crop, self.resize, 1, self.device)

    def _finish(self, lengths, records):
        if self._single:                        # CarlaSeg: every frame is a sample (n + 1 frames of past 1, future 0: n windows)
            self.index = SequenceIndex([sum(lengths) + 1], 1, 0, self.seed)
            self.index.masks = self.index.frames
        else:
            self.index = SequenceIndex(lengths, self.past_frames, self.future_frames, self.seed)
        self.indices = self.index.indices
        self.table = None
        for s in (self.store, self.mask_store):
            if s is not None:
                s.release_staging()
        if self.load_measurements:
            self.table_cpu = measurement_table(records, self.speed_factor, self.n_commands)
            if len(self.index):                 # uploaded once
                self.table = self.table_cpu.to(self.store.device)

    def __len__(self):
        return len(self.index)

    # ---- batches
    def _augmenter(self):
        return get_augmenter(self.boost * self.samples_read, self.batch_size, self.aug_type)

    def _sample_ids(self, sample_ids):
        ids = torch.as_tensor(sample_ids, dtype=torch.int64, device="cpu").reshape(-1)
        if ids.numel() < 1:
            raise ValueError("batch: no sample ids")
        if int(ids.min()) < 0 or int(ids.max()) >= len(self):
            raise IndexError(f"batch: sample ids must be in [0, {len(self)}), got {int(ids.min())} .. {int(ids.max())}")
        return ids

    def batch(self, sample_ids, plan=None, generator=None):
        """The one place a batch is made.  ``sample_ids``: positions in ``indices`` (what ``dataset[i]`` takes), checked on the
        host.  The index tables go up in one pinned non-blocking copy.  ``mode="val"``: one ``pmoe_gather_frames_to_f32`` launch.
        ``mode="train"``: ``pmoe_gather_rows`` into a uint8 staging tensor, then the augmenter's launches
        (``augment.run_plan``; its last one is ToTensor); the augmenter is ``get_augmenter(boost * samples_read_so_far,
        batch_size, aug_type)``, built once per batch (the module docstring says how that differs from the reference), the plan
        has one row per FRAME -- each frame of a window draws independently, as in the reference -- and is drawn from
        ``generator`` unless ``plan`` (an ``AugmentPlan`` of ``B * T`` rows) is given.  The targets are one ``pmoe_gather_rows``
        over the measurement table, or one ``pmoe_gather_labels_to_i64``."""
        ids = self._sample_ids(sample_ids)
        win = self.indices[ids]
        B, T = int(ids.numel()), self.index.frames.shape[1]
        h, w = self.store.h, self.store.w
        f_ids = self.index.frames[win].reshape(-1)
        t_ids = (self.index.measurement[win] if self.load_measurements else self.index.masks[win]).reshape(-1)
        nt = int(t_ids.numel())
        if plan is not None and self.mode != "train":
            raise ValueError("batch: a plan needs mode='train'")
        if self.mode == "train":                # the plan first: a refused one launches nothing
            plan = self._augmenter()._plan_for(B * T, h, w, generator, plan)
        dev = self.store.device
        with torch.cuda.device(dev):
            host = torch.empty(B * T + nt, dtype=torch.int64, pin_memory=True)
            host[:B * T], host[B * T:] = f_ids, t_ids
            tbl = host.to(dev, non_blocking=True)
            f_tbl, t_tbl = tbl[:B * T], tbl[B * T:]
            if self.mode == "train":
                stage = gather_rows(self.store.data, f_tbl, self.store.count)
                img = torch.empty(B * T, 3, h, w, dtype=torch.float32, device=dev)
                run_plan(stage, plan, img)
            else:
                img = gather_frames_to_f32(self.store.data, f_tbl, self.store.count)
            self.samples_read += B
            img = img.view(B, 3, h, w) if self._single else img.view(B, T, 3, h, w)
            if self.load_measurements:
                rows = gather_rows(self.table, t_tbl)
                return img, {"control": rows[:, 0:2].contiguous(), "speed": rows[:, 2].contiguous(),
                             "target_speed": rows[:, 3].contiguous(), "command": rows[:, 4:].contiguous()}
            masks = gather_labels_to_i64(self.mask_store.data, t_tbl, self.mask_store.count).view(nt, h, w)
            return img, (masks.view(B, h, w) if self._single else masks.view(B, nt // B, h, w))

    def loader(self, batch_size=None, shuffle=False, drop_last=False, generator=None, rank=0, world=1, **ignored):
        """An iterable of ``ds.batch`` results with ``len`` = the batch count, for the place of ``DataLoader(ds, ...)``:
        ``num_workers``, ``pin_memory``, ``worker_init_fn`` and the like are accepted and ignored.  ``shuffle`` draws
        ``torch.randperm(len(ds), generator=generator)`` per epoch (not the stream of ``DataLoader``'s sampler); ``generator`` also
        feeds the train-mode plans.  ``rank`` / ``world`` cut each global batch with ``parallel.shard_batch``."""
        return _Loader(self, self.batch_size if batch_size is None else batch_size, shuffle, drop_last, generator, rank, world)


class CarlaSeg(CarlaSegPred):
    """``CarlaSeg(root, aug_type, mode, seed, crop, resize)`` of the reference (``data_loader.py:45-129``): every frame is a
    sample, ``img [B, 3, h, w]`` and ``mask [B, h, w]``.  The frames and the masks of all episodes are paired by their sorted full
    paths, as there.  Train mode augments the frame only; the reference builds its augmenter once (``iteration=None``, which only
    the ``segmentation`` type accepts), and so the schedule here stays at iteration 0 (``boost=0``)."""

    _single = True

    def __init__(self, root="../data/train", aug_type="segmentation", mode="train", seed=0, crop=(125, 90), resize=(224, 224),
                 batch_size=32, device="cuda"):
        super().__init__(root, 1, 0, aug_type, mode, seed, False, batch_size, 0, crop, resize, device=device)

    @classmethod
    def from_arrays(cls, episodes, aug_type="segmentation", mode="train", seed=0, crop=(125, 90), resize=(224, 224),
                    batch_size=32, device="cuda"):
        return super().from_arrays(episodes, 1, 0, aug_type, mode, seed, False, batch_size, 0, crop, resize, device=device)
