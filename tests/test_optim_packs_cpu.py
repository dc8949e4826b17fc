"""The tile table of mt_adam_pack_kernel (pmoe_amd.optim.pack_tiles) is a pure function of the tensor shapes: every (co, ci,
tap) of every tensor belongs to exactly one tile, no tile crosses a tensor, every tile fits the LDS stage, and the extents give
both packed operands contiguous runs of >= 32 bytes wherever the layer has the channels."""
import ctypes

import numpy as np

from pmoe_amd import optim

# (cout, cin, taps): the layers of tests/test_optim_packs_gpu.py, then what else the networks hold
SHAPES = [(64, 12, 9), (5, 1536, 1), (130, 70, 9), (128, 256, 9), (130, 1, 1), (4, 1536, 1), (1, 1536, 1),
          (512, 512, 9), (512, 1536, 1), (64, 1, 1), (1, 1, 1), (23, 64, 1), (64, 138, 9), (32, 16, 49), (17, 33, 25),
          (256, 128, 4), (4096, 1, 1), (5000, 1, 1)]


def test_tiles_partition_every_tensor():
    dims, tt, c0, i0 = optim.pack_tiles(SHAPES)
    assert len(dims) == len(SHAPES) and len(tt) == len(c0) == len(i0)
    seen = [np.zeros((cout, cin, taps), dtype=np.int32) for cout, cin, taps in SHAPES]
    for t, co0, ci0 in zip(tt, c0, i0):
        cout, cin, taps = SHAPES[t]
        tco, tci = dims[t]
        assert 0 <= co0 < cout and 0 <= ci0 < cin, "a tile starts inside its tensor"
        rows, cols = min(tco, cout - co0), min(tci, cin - ci0)
        assert rows >= 1 and cols >= 1
        assert rows * ((cols * taps) | 1) <= optim.PACK_STAGE, "the tile fits the LDS stage"
        seen[t][co0:co0 + rows, ci0:ci0 + cols, :] += 1         # (slices clamp: the explicit min above is what the kernel does)
    for t, s in enumerate(seen):
        assert (s == 1).all(), (SHAPES[t], int(s.min()), int(s.max()))


def test_tile_extents_give_32_byte_runs():
    for cout, cin, taps in SHAPES:
        tco, tci = optim.pack_tile_dims(cout, cin, taps)
        assert tco * ((min(tci, cin) * taps) | 1) <= optim.PACK_STAGE
        assert tci >= 16                                        # forward operand: runs of min(tci, cin) elements along ci
        if taps <= 9:                                           # the filters the networks have: 16 co rows fit the stage
            assert tco >= 16 and tco % 16 == 0                  # data-gradient operand: runs of min(tco, cout) along co
    assert optim.pack_tile_dims(512, 512, 9) == (16, 32)
    assert optim.pack_tile_dims(512, 1536, 1) == (16, 288)


def test_tiles_are_a_pure_function_of_the_shapes():
    assert optim.pack_tiles(SHAPES) == optim.pack_tiles(list(SHAPES))
    one = optim.pack_tiles([SHAPES[2]])
    assert one[1] == [0] * len(one[1]) and len(one[1]) == -(-130 // one[0][0][0]) * -(-70 // one[0][0][1])


def test_pack_row_layout():
    assert ctypes.sizeof(optim.OptPack) == optim._PACK_ROW.itemsize == 64
    for name, _ in optim.OptPack._fields_:
        assert getattr(optim.OptPack, name).offset == optim._PACK_ROW.fields[name][1], name
    assert ctypes.sizeof(optim.OptTensor) == 64                 # the rows the packs run parallel to keep their size


def test_entry_point_is_exported_and_checks_its_arguments():
    from pmoe_amd import hip
    if not hip.lib_path().exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = hip.load()
    assert lib.pmoe_abi_sizeof(3) == ctypes.sizeof(optim.OptPack)
    assert lib.pmoe_abi_sizeof(2) == 64 and lib.pmoe_version() == 401
    for n_tiles, ptr in ((1, None), (0, 0x1000)):              # (refused before any launch: runs without a GPU)
        assert lib.pmoe_mt_adam_packs(ptr, ptr, ptr, ptr, ptr, n_tiles, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0.1, 0.1, None,
                                      None) == hip.ERR_ARG
