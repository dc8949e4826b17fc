"""Device-resident dataset on the MI355X (pmoe_amd/data.py, csrc/dataset.hip): the Resize output against the Pillow fixtures, the
three gathers against torch indexing (bit exact; the 16-byte, 4-byte and byte paths, unaligned views, a store beyond 4 GiB), and
the datasets end to end against FramePreprocessor run by hand on the raw frames of each window."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.make_prep_golden import CASES, frame, mask  # noqa: E402
from pmoe_amd import data, hip  # noqa: E402
from pmoe_amd.augment import AugmentPlan, get_augmenter  # noqa: E402
from pmoe_amd.data import CarlaSeg, CarlaSegPred, FrameStore, measurement_table  # noqa: E402
from pmoe_amd.preprocess import FramePreprocessor  # noqa: E402


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_resized_is_the_pillow_resize_output(golden_dir, case):
    name, H0, W0, crop, size, seed = case
    want = torch.from_numpy(np.load(golden_dir / "prep.npz")[name])
    fr = torch.from_numpy(frame(H0, W0, seed)).cuda()
    pre = FramePreprocessor(crop, size)
    got = pre.resized(fr)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(size) + (3,)
    assert torch.equal(got.cpu(), want)
    both = pre.resized(torch.stack([fr.flip(0), fr]))
    assert tuple(both.shape) == (2,) + tuple(size) + (3,) and torch.equal(both[1].cpu(), want)
    with pytest.raises(TypeError):
        pre.resized(fr.float())
    with pytest.raises(RuntimeError, match="no CPU path"):
        pre.resized(fr.cpu())


# ---- the gathers against torch indexing
N = 37


def _to_tensor(u8_nhwc):
    """ToTensor of gathered frames, divided on the host: torch divides by a scalar on the device as a multiplication by its
    reciprocal, which is not the division ToTensor (and the kernels) do"""
    return u8_nhwc.cpu().permute(0, 3, 1, 2).float() / 255


def _idx(n, n_src, seed):
    """n indices into [0, n_src): repeats, and (from n = 2) both 0 and n_src - 1"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n_src, (n,), generator=g)
    idx[0] = n_src - 1
    if n > 1:
        idx[1] = 0
    if n > 3:
        idx[3] = idx[2]
    return idx.cuda()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one_byte_in"])
@pytest.mark.parametrize("hw", [(32, 32), (6, 6), (7, 5)], ids=["row3072", "row108", "row105"])
def test_gathers_equal_torch_indexing(hw, offset):
    h, w = hw
    row = h * w * 3
    g = torch.Generator().manual_seed(row + offset)
    buf = torch.randint(0, 256, (N * row + 16,), dtype=torch.uint8, generator=g).cuda()
    store = buf[offset:offset + N * row].view(N, h, w, 3)
    assert store.data_ptr() % 16 == offset
    labels = store.view(N, row)
    for n in (1, 5, 130):
        idx = _idx(n, N, n)
        got = data.gather_rows(store, idx)
        assert got.dtype == torch.uint8 and torch.equal(got, store[idx])
        f32 = data.gather_frames_to_f32(store, idx)
        assert f32.dtype == torch.float32 and tuple(f32.shape) == (n, 3, h, w)
        assert torch.equal(f32.cpu(), _to_tensor(store[idx]))
        i64 = data.gather_labels_to_i64(labels, idx)
        assert i64.dtype == torch.int64 and torch.equal(i64, labels[idx].long())
    # single-channel frames (the mask store's layout) and a channel count the 4-pixel path is not compiled for
    for c in (1, 2):
        st = buf[offset:offset + N * h * w * c].view(N, h, w, c)
        idx = _idx(5, N, c)
        assert torch.equal(data.gather_frames_to_f32(st, idx).cpu(), _to_tensor(st[idx]))


@pytest.mark.parametrize("width", [10, 4, 3])
def test_gather_rows_of_f32_measurements(width):
    table = torch.randn(N, width, generator=torch.Generator().manual_seed(width)).cuda()
    for n in (1, 5, 130):
        idx = _idx(n, N, 10 * n)
        assert torch.equal(data.gather_rows(table, idx), table[idx])


def test_rows_outside_the_filled_part_come_back_as_zeros():
    """the kernels' own guard (the Python side never sends such an index): an index outside [0, n_src) reads nothing"""
    store = torch.randint(1, 256, (N, 6, 6, 3), dtype=torch.uint8).cuda()
    idx = torch.tensor([0, 20, -1, 36, 19, 1 << 40], dtype=torch.int64).cuda()
    keep = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.bool).cuda()            # n_src = 20
    want = store[idx.clamp(0, N - 1)] * keep[:, None, None, None]
    assert torch.equal(data.gather_rows(store, idx, n_src=20), want)
    assert torch.equal(data.gather_frames_to_f32(store, idx, n_src=20).cpu(), _to_tensor(want))
    assert torch.equal(data.gather_labels_to_i64(store, idx, n_src=20), want.long())


def test_gathers_from_a_store_larger_than_4_gib():
    """22,000 frames of 256 x 256 x 3 = 4.3 GB: the last rows lie beyond a 32-bit byte offset"""
    rows, h, w = 22000, 256, 256
    store = torch.empty(rows, h, w, 3, dtype=torch.uint8, device="cuda")
    assert store.numel() > (1 << 32)
    used = [0] + list(range(rows - 8, rows))
    fill = torch.randint(0, 256, (len(used), h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    for k, r in enumerate(used):
        store[r] = fill[k]
    idx = torch.tensor([rows - 1, 0, rows - 8, rows - 3, rows - 3, rows - 5, rows - 2, rows - 4, rows - 6, rows - 7]).cuda()
    want = fill[torch.tensor([used.index(int(r)) for r in idx.tolist()]).cuda()]
    assert torch.equal(data.gather_rows(store, idx), want)
    assert torch.equal(data.gather_frames_to_f32(store, idx).cpu(), _to_tensor(want))
    assert torch.equal(data.gather_labels_to_i64(store.view(rows, -1), idx), want.view(len(idx), -1).long())
    del store


# ---- end to end
LENGTHS, H0, W0, CROP, SIZE, PAST, FUTURE = (13, 12), 60, 80, (10, 6), (32, 32), 4, 2


def _windows():
    """(frame ids, measurement id, mask ids) of every window, written out (data_loader.py:191-196)"""
    out, base = [], 0
    for L in LENGTHS:
        for i in range(L - (PAST + FUTURE)):
            out.append((list(range(base + i, base + i + PAST)), base + i + PAST,
                        list(range(base + i + PAST, base + i + PAST + FUTURE))))
        base += L
    return out


@pytest.fixture(scope="module")
def world():
    """the raw episodes once, and what FramePreprocessor makes of every frame and mask"""
    rng = np.random.default_rng(3)
    raw = np.stack([frame(H0, W0, 100 + k) for k in range(sum(LENGTHS))])
    raw_masks = np.stack([mask(H0, W0, 200 + k, block=5) for k in range(sum(LENGTHS))])
    records = [dict(steer=float(rng.uniform(-1, 1)), brake=float(rng.choice([0.0, 0.05, 0.4])), throttle=float(rng.uniform(0, 1)),
                    speed=float(rng.uniform(0, 30)), target_speed=float(rng.uniform(0, 30)), command=int(rng.integers(1, 5)))
               for _ in range(sum(LENGTHS))]
    cuts = np.cumsum((0,) + LENGTHS)
    episodes = [dict(rgb=raw[a:b], mask=raw_masks[a:b], measurements=records[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pre = FramePreprocessor(CROP, SIZE)
    raw_dev, masks_dev = torch.from_numpy(raw).cuda(), torch.from_numpy(raw_masks).cuda()
    return dict(episodes=episodes, records=records, pre=pre, raw=raw_dev, raw_masks=masks_dev, frames=pre(raw_dev),
                labels=pre.labels(masks_dev), windows=_windows())


def _pred(world, **kw):
    return CarlaSegPred.from_arrays(world["episodes"], PAST, FUTURE, crop=CROP, resize=SIZE, **kw)


def test_store_appends_host_and_device_frames_alike(world):
    raw = world["raw"]
    store = FrameStore(30, CROP, SIZE)
    assert store.append(raw[:3]) == range(0, 3)                         # device tensor
    assert store.append(raw[3:9].cpu()) == range(3, 9)                  # CPU tensor
    assert store.append(raw[9:25].cpu().numpy()) == range(9, 25)        # numpy
    assert store.append(raw[0]) == range(25, 26)                        # one frame
    assert len(store) == 26 and torch.equal(store.data[:25], world["pre"].resized(raw)) and torch.equal(store.data[25], store.data[0])
    with pytest.raises(ValueError, match="capacity"):
        store.append(raw[:5])
    with pytest.raises(ValueError, match="60 x 80"):
        store.append(raw[:1, :50])
    assert len(store) == 26
    masks = FrameStore(25, CROP, SIZE, channels=1)
    assert masks.append(world["raw_masks"].cpu()) == range(0, 25)
    assert torch.equal(masks.data[..., 0].long(), world["labels"])


def test_measurements_form_end_to_end(world):
    ds = _pred(world, mode="val", load_measurements=True, seed=4)
    wins, table = world["windows"], measurement_table(world["records"]).cuda()
    assert len(ds) == len(wins) == 13
    loader = ds.loader(5, shuffle=False, num_workers=4, pin_memory=True)
    assert len(loader) == 3
    sizes, seen = [], 0
    with hip.LaunchRecorder() as rec:
        batches = list(loader)
    assert [fn.__name__ for fn, _ in rec.calls] == ["pmoe_gather_frames_to_f32", "pmoe_gather_rows"] * 3
    for img, meas in batches:
        B = img.shape[0]
        sizes.append(B)
        assert img.dtype == torch.float32 and tuple(img.shape) == (B, PAST, 3) + SIZE and img.is_cuda
        assert tuple(meas["control"].shape) == (B, 2) and tuple(meas["speed"].shape) == (B,)
        assert tuple(meas["target_speed"].shape) == (B,) and tuple(meas["command"].shape) == (B, 4)
        for b in range(B):
            f_ids, m_id, _ = wins[int(ds.indices[seen + b])]              # shuffle=False: the order is `indices`
            for t in range(PAST):
                assert torch.equal(img[b, t], world["frames"][f_ids[t]])
            assert torch.equal(meas["control"][b], table[m_id, :2]) and meas["speed"][b] == table[m_id, 2]
            assert meas["target_speed"][b] == table[m_id, 3] and torch.equal(meas["command"][b], table[m_id, 4:])
        seen += B
    assert sizes == [5, 5, 3]                                           # the last batch is short
    assert len(ds.loader(5, drop_last=True)) == 2
    # a shuffled epoch is a permutation of the same samples; two ranks split each global batch
    g = torch.Generator().manual_seed(9)
    order = torch.randperm(13, generator=torch.Generator().manual_seed(9))
    first = next(iter(ds.loader(4, shuffle=True, generator=g)))[0]
    assert torch.equal(first, ds.batch(order[:4])[0])
    halves = [next(iter(ds.loader(4, rank=r, world=2)))[0] for r in (0, 1)]
    assert torch.equal(torch.cat(halves), ds.batch(range(4))[0])


def test_train_mode_is_the_augmented_pipeline_bit_for_bit(world):
    ds = _pred(world, mode="train", load_measurements=True, aug_type="super_hard", batch_size=5, boost=3)
    ids = [0, 1, 2, 3, 4]
    blur, point = [{"op": "blur", "sigma": 1.2}], [{"op": "add", "p": (40, -17, 3)}, {"op": "multiply", "p": 1.5}]
    mixed = [{"op": "contrast", "p": 0.5}, {"op": "blur", "sigma": 2.0}, {"op": "dropout", "p": 0.3, "seed": 5, "per_channel": 1}]
    slots = [[blur, [], point, mixed][k % 4] for k in range(5 * PAST)]
    plan = AugmentPlan.from_slots(slots, *SIZE)
    f_ids = torch.tensor([world["windows"][int(ds.indices[i])][0] for i in ids]).cuda()
    aug = get_augmenter(0, 5, "super_hard")
    want = world["pre"](world["raw"][f_ids], augment=aug, plan=plan)
    with hip.LaunchRecorder() as rec:
        img, _ = ds.batch(ids, plan=plan)
    assert [fn.__name__ for fn, _ in rec.calls][0] == "pmoe_gather_rows" and rec.calls[-1][0].__name__ == "pmoe_gather_rows"
    assert tuple(img.shape) == (5, PAST, 3) + SIZE and torch.equal(img, want)
    flat, val = img.view(-1, 3, *SIZE), world["frames"][f_ids.view(-1)]
    changed = [not torch.equal(flat[k], val[k]) for k in range(5 * PAST)]
    assert changed == [bool(s) for s in slots]                          # a frame with no slot equals the val-mode frame
    # drawn plans: one row per frame, the schedule from boost * samples read so far, the draws from the generator given
    assert ds.samples_read == 5
    g1, g2 = torch.Generator().manual_seed(2), torch.Generator().manual_seed(2)
    drawn = get_augmenter(3 * 5, 5, "super_hard").plan(5 * PAST, *SIZE, generator=g2)
    got, _ = ds.batch(ids, generator=g1)
    assert ds.samples_read == 10
    assert torch.equal(got, world["pre"](world["raw"][f_ids], augment=aug, plan=drawn))
    with pytest.raises(ValueError, match="plan"):
        ds.batch(ids, plan=AugmentPlan.empty(3, *SIZE))
    with pytest.raises(ValueError, match="plan"):
        _pred(world, mode="val").batch(ids, plan=plan)


def test_masks_form_end_to_end(world):
    ds = _pred(world, mode="val", load_measurements=False, seed=1)
    wins, seen = world["windows"], 0
    for img, masks in ds.loader(5):
        B = img.shape[0]
        assert masks.dtype == torch.int64 and tuple(masks.shape) == (B, FUTURE) + SIZE and tuple(img.shape) == (B, PAST, 3) + SIZE
        for b in range(B):
            f_ids, _, k_ids = wins[int(ds.indices[seen + b])]
            assert torch.equal(img[b], world["frames"][torch.tensor(f_ids).cuda()])
            assert torch.equal(masks[b], world["pre"].labels(world["raw_masks"][torch.tensor(k_ids).cuda()]))
        seen += B
    assert seen == 13
    seg = CarlaSeg.from_arrays(world["episodes"], mode="val", crop=CROP, resize=SIZE, seed=2)
    assert len(seg) == sum(LENGTHS)
    state = torch.random.get_rng_state()
    torch.random.manual_seed(2)
    order = torch.randperm(sum(LENGTHS))
    torch.random.set_rng_state(state)
    assert torch.equal(seg.indices, order)
    batches = list(seg.loader(8))
    assert [b[0].shape[0] for b in batches] == [8, 8, 8, 1]
    img, masks = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
    assert tuple(img.shape) == (25, 3) + SIZE and tuple(masks.shape) == (25,) + SIZE and masks.dtype == torch.int64
    assert torch.equal(img, world["frames"][order.cuda()]) and torch.equal(masks, world["labels"][order.cuda()])
    train = CarlaSeg.from_arrays(world["episodes"], mode="train", crop=CROP, resize=SIZE)
    timg, tmasks = train.batch(range(8), generator=torch.Generator().manual_seed(0))
    assert tuple(timg.shape) == (8, 3) + SIZE and torch.equal(tmasks, world["labels"][train.indices[:8].cuda()])


def test_a_training_step_fed_from_the_loader_gives_the_same_loss_bits():
    """the g1-sized mixture (4 experts, B = 2, T = 4, 128 x 128, 6 commands): model(img, speed.unsqueeze(-1), command), moe_loss,
    backward -- fed from the loader and from tensors assembled by hand with FramePreprocessor"""
    from oracle import pmoe_oracle as O
    from pmoe_amd.loss import moe_loss
    from tests.parity_util import GOLDEN, build_pair
    g = torch.load(GOLDEN / "g1_moe_e4_b2_128.pt", weights_only=False)
    ocfg, _, model, _ = build_pair(g, torch.float32)
    rng = np.random.default_rng(11)
    L, crop, size = 6, (20, 12), (128, 128)
    raw = np.stack([frame(160, 176, 300 + k) for k in range(L)])
    records = [dict(steer=float(rng.uniform(-1, 1)), brake=0.0, throttle=float(rng.uniform(0, 1)), speed=float(rng.uniform(0, 10)),
                    target_speed=float(rng.uniform(0, 10)), command=int(rng.integers(1, 7))) for _ in range(L)]
    ds = CarlaSegPred.from_arrays([dict(rgb=raw, measurements=records)], 4, 0, mode="val", load_measurements=True, batch_size=2,
                                  crop=crop, resize=size, n_commands=6)
    assert len(ds) == 2

    def step(img, control, speed, target_speed, command):
        model.zero_grad(set_to_none=True)
        dist, speeds = model(img, speed, command)
        loss = moe_loss(dist, speeds, control, target_speed, ocfg.loss_coefs)
        loss.backward()
        return loss.detach().clone()

    (img, meas), = list(ds.loader(2))
    got = step(img, meas["control"], meas["speed"].unsqueeze(-1), meas["target_speed"].unsqueeze(-1), meas["command"])
    order = [int(ds.indices[i]) for i in range(2)]                      # window (= its first frame) of sample 0 and 1
    pre = FramePreprocessor(crop, size)
    raw_dev = torch.from_numpy(raw).cuda()
    hand_img = torch.stack([pre(raw_dev[w:w + 4]) for w in order])
    mid = [w + 4 for w in order]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).cuda()        # noqa: E731
    control = f32([[records[m]["steer"], records[m]["throttle"]] for m in mid])
    speed = f32([[records[m]["speed"] / 10] for m in mid])
    target_speed = f32([[records[m]["target_speed"] / 10] for m in mid])
    command = torch.nn.functional.one_hot(torch.tensor([records[m]["command"] - 1 for m in mid]), 6).float().cuda()
    assert torch.equal(hand_img, img) and torch.equal(control, meas["control"]) and torch.equal(command, meas["command"])
    assert torch.equal(speed, meas["speed"].unsqueeze(-1)) and torch.equal(target_speed, meas["target_speed"].unsqueeze(-1))
    want = step(hand_img, control, speed, target_speed, command)
    assert torch.isfinite(got) and got.item() == want.item()
