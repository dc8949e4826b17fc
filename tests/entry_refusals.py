"""Calls that the pass-kernel entry points of the library refuse with PMOE_ERR_ARG before any launch: one or more for every
``return PMOE_ERR_ARG`` that an entry point of elementwise / stem_tail / heads / punet / stage1 / stage0 / optim / preprocess /
augment.hip can reach.  Every row is the entry point's accepted argument list with the one change that trips one check, so no
earlier check fires first.  tests/test_entry_refusals_cpu.py compares this tree's return codes with
tests/golden/entry_refusals.json;

    PMOE_HIP_LIB=<libpmoe_hip.so of a revision> python tests/entry_refusals.py tests/golden/entry_refusals.json

writes the fixture from the library of ANY revision (the committed file: the revision before the entry points shared one dtype
dispatch, grid rule and launch call).  Device pointers are small made-up integers: a refused call dereferences nothing.  What the
host reads before its checks is real host memory: the 12-entry ``consts`` array ("host12") and the source-pointer array of
pmoe_cat_windows ("host8")."""
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.append(str(ROOT))

BAD_DT = 7                                   # neither PMOE_DT_BF16 (0) nor PMOE_DT_F32 (1)
p1, p2, p3, p4, p5, p6, p7, p8, p9, p10, p11, p12 = (0x1000 * k for k in range(1, 13))      # 16-byte aligned, never dereferenced
BIG = 65536


def _window(ld, coff):
    """the three ways a channel window of 64 bf16 channels is refused: row width, offset, overhang"""
    return [{ld: 68}, {ld: 128, coff: 4}, {ld: 64, coff: 8}]


def _chanvec(c):
    """C = 64 bf16 channels -> no multiple of the vector, 3 vectors (no power of two), 512 vectors (> 256)"""
    return [{c: 60}, {c: 24}, {c: 4096}]


def _nulls(*idx):
    return [{i: None} for i in idx]


_window_copy = ([p1, 64, 0, p2, 64, 0, 16, 64, 0, None], [{6: -1}, {7: 0}, {2: 8}, {5: 8}, {8: BAD_DT}])
_vertical = ([p1, p2, 2, 8, 8, 3, 4, p3, p4, 3, None], _nulls(0, 1, 7, 8) + [{2: 0}, {3: 0}, {4: 0}, {5: 0}, {6: 0}, {9: 0}])
_point = ([p1, p2, p3, 1, 8, 8, 0, None], _nulls(0, 1, 2) + [{3: 0}, {3: BIG}, {4: 0}, {5: 0}, {6: 2}, {6: -1}, {4: 32768, 5: 16384}])
_blur = ([p1, p2, p3, 1, 8, 8, None], _nulls(0, 1, 2) + [{3: 0}, {4: 0}, {5: 0}, {1: p1}, {4: 1 << 22, 5: 1}])
_packs = _nulls(0, 1, 2, 3, 4) + [{5: 0}]

# entry point -> (accepted arguments, [{argument index: value that is refused}, ...])
CASES = {
    # ---- elementwise.hip
    "pmoe_colstats": ([p1, 64, 2, 64, 64, 0, p2, 4, p3, 0, None],
                      _chanvec(3) + [{7: 0}, {1: 0}, {2: 0}, {5: -8}, {9: BAD_DT}, {9: 1, 3: 62}] + _window(4, 5)),
    "pmoe_bn_bwd_reduce": ([p1, p2, p3, p4, p5, p6, p7, 64, 2, 64, 1, p8, 4, p9, 0, None],
                           [{1: None, 5: None}, {1: None, 6: None}, {12: 0}, {14: BAD_DT}] + _chanvec(9)),
    "pmoe_reduce_partials": ([p1, p2, 2, 4, 2, 64, None], [{3: 0}, {4: 0}, {5: 0}]),
    "pmoe_bn_finalize": ([p1, 4, 128, p2, p3, p4, p5, 0.125, 0.5, 1, p6, p7, p8, p9, 2, 64, p10, None],
                         [{9: 0, 5: None}, {9: 0, 6: None}]),
    "pmoe_bn_apply": ([p1, None, p2, p3, p4, p5, 64, 2, 64, 1, 0, 0, 0, None, 1.0, None],
                      _chanvec(8) + [{13: p6, 12: 1}, {13: p6, 10: 128}, {12: BAD_DT}, {12: 1, 8: 62}] + _window(10, 11)),
    "pmoe_bn_apply_pool2": ([p1, p2, p3, p4, p5, p6, 2, 8, 8, 2, 64, 1, 0, 0, 0, None],
                            _nulls(0, 1, 2) + [{6: 0}, {9: 0}, {7: 0}, {8: 0}, {7: 7}, {8: 7}, {14: BAD_DT}] + _chanvec(10) + _window(12, 13)),
    "pmoe_bn_bwd_apply": ([p1, p2, p3, p4, p5, p6, p7, p8, p9, p10, p11, 64, 2, 64, 1, 0, None], _chanvec(13) + [{15: BAD_DT}, {15: 1, 13: 62}]),
    "pmoe_act_fwd": ([p1, p2, 64, 1, 0.0, 5, 0, None],
                     _nulls(0, 1) + [{2: 0}, {3: -1}, {3: 5}, {4: -0.5}, {4: 1.0}, {2: 60}, {6: 1, 2: 62}, {6: BAD_DT}]),
    "pmoe_act_bwd": ([p1, p2, p3, 64, 1, 0.0, 0, None],
                     _nulls(0, 1, 2) + [{3: 0}, {4: -1}, {4: 5}, {5: -0.5}, {5: 1.0}, {3: 60}, {6: 1, 3: 62}, {6: BAD_DT}]),
    "pmoe_maxpool3s2_fwd": ([p1, p2, p3, 2, 8, 8, 64, 0, None], [{6: 60}, {7: 1, 6: 62}, {7: BAD_DT}]),
    "pmoe_maxpool3s2_bwd": ([p1, p2, p3, 2, 8, 8, 64, 0, None], [{6: 60}, {7: 1, 6: 62}, {7: BAD_DT}]),
    "pmoe_gap_partial": ([p1, None, p2, 2, 64, 64, 4, 0, 0, None], [{5: 60}, {5: 4096}, {6: 0}, {8: BAD_DT}]),
    "pmoe_bn_apply_gap": ([p1, p2, p3, p4, p5, p6, 4, 4, 2, 64, 64, 1, 0, None],
                          _nulls(0, 1, 2, 3, 4, 5) + [{6: 0}, {7: 0}, {8: 0}, {8: 3}, {9: 0}, {10: 60}, {10: 4096}, {12: BAD_DT}]),
    "pmoe_gap_finish": ([p1, p2, 2, 64, 4, 64, 64, 0, 0, None], [{8: BAD_DT}]),
    "pmoe_gap_bwd": ([p1, p2, 2, 64, 64, 64, 0, 0, None], [{4: 60}, {5: 68}, {6: 4}, {7: BAD_DT}]),
    "pmoe_eca_gate": ([p1, 4, 64, p2, 3, p3, p4, 4, 2, 0, 64, 64, None], [{10: 2048}, {4: 11}, {4: 0}, {4: 4}]),
    "pmoe_eca_scale": ([p1, p2, p3, 2, 64, 64, 0, 0, None], [{5: 60}, {7: BAD_DT}]),
    "pmoe_eca_bwd_small": ([p1, 4, p2, p3, p4, 3, p5, p6, p7, 4, 2, 64, 64, 1.0, None], [{11: 2048}, {5: 11}, {5: 0}, {9: 3}, {8: None}]),
    "pmoe_eca_bwd_apply": ([p1, p2, p3, p4, 2, 64, 64, 0, None], [{6: 60}, {7: BAD_DT}]),
    "pmoe_nchw_to_nhwc": ([p1, p2, 2, 3, 8, 8, 8, 0, None], [{2: 0}, {3: 0}, {4: 0}, {5: 0}, {6: 2}, {7: BAD_DT}]),
    "pmoe_pad_rows": ([p1, p2, 2, 5, 8, 0, None], [{5: BAD_DT}]),
    # ---- stem_tail.hip (the walk kernels' workgroup count: 2^16 images of 2^16 x 2^16 pixels)
    "pmoe_stem_tail_stats": ([p1, p2, p3, p4, p5, 4, p6, p7, 2, 2, 8, 8, 64, 0, None],
                             _chanvec(12) + [{5: 0}, {13: BAD_DT}, {13: 1, 12: 62}]),
    "pmoe_stem_tail_pool": ([p1, p2, p3, p4, p5, p6, p7, p8, p9, 4, 2, 8, 8, 64, 0, None],
                            _chanvec(13) + [{9: 3}, {9: BIG, 10: 1, 11: BIG, 12: BIG}, {14: BAD_DT}, {14: 1, 13: 62}]),
    "pmoe_stem_tail_bwd": ([1, p1, p2, p3, p4, "host12", p5, 4, 2, 2, 8, 8, 64, 0, None],
                           _chanvec(12) + [{7: 0}, {0: 0}, {0: 4}, {0: 3, 8: BIG, 9: 1, 10: BIG, 11: BIG}, {0: 3, 13: BAD_DT},
                                           {0: 1, 13: BAD_DT}, {0: 2, 13: BAD_DT}, {13: 1, 12: 62}]),
    "pmoe_stem_tail_pooled": ([p1, p2, p3, "host12", p4, 4, 2, 64, 64, 0, None], _chanvec(8) + [{5: 0}, {7: 0}, {9: BAD_DT}, {9: 1, 8: 62}]),
    "pmoe_stem_tail_combine": ([p1, 4, p2, 4, "host12", 128, p3, p4, 2, 64, None], [{1: 0}, {3: 0}, {5: 0}]),
    # ---- heads.hip
    "pmoe_pack_conv_weights_fp8": ([p1, p2, p3, p4, p5, 1.0, 2, 8, 8, 3, 16, 16, 16, 16, None],
                                   _nulls(0, 3, 4) + [{5: 0.0}, {10: 4}, {11: 4}, {12: 4}, {13: 4}]),
    "pmoe_pack_conv_weights": ([p1, p2, p3, 2, 8, 8, 3, 16, 16, 16, 16, 0, None],
                               [{7: 4}, {8: 4}, {9: 4}, {10: 4}, {7: 16384, 8: 16384}, {11: BAD_DT}]),
    "pmoe_pack_conv_weights_gated": ([p1, p2, 8, p3, p4, 4, 2, 8, 8, 3, 16, 16, 16, 16, 0, None],
                                     [{5: 0}, {6: 0}, {5: 3}, {10: 4}, {11: 4}, {2: 4}, {1: None}, {12: 4}, {13: 4}, {14: BAD_DT}]),
    "pmoe_pack_conv_weights_scaled": ([p1, p2, p3, p4, p5, p6, 2, 8, 8, 3, 16, 16, 0, None],
                                      _nulls(1, 2, 3, 4, 5) + [{6: 0}, {10: 4}, {11: 4}, {12: BAD_DT}]),
    "pmoe_eca_stem_fold": ([p1, p2, p3, p4, p5, 4, 2, 8, 8, 3, 16, 16, 8, None], [{5: 3}, {12: 512}, {11: 4}, {12: 4}, {10: 4}]),
    "pmoe_gate_mixture_fwd": ([p1, 8, p2, 4, p3, p4, p5, p6, 4, 4, 0, 0, 0, None], [{9: 0}, {9: 65}, {1: 4}, {11: 1}, {12: BAD_DT}]),
    "pmoe_gate_mixture_bwd": ([p1, 8, p2, p3, p4, p5, p6, p7, p8, 4, 4, 4, 0, 0, 0, None], [{11: 0}, {11: 65}, {1: 4}, {13: 1}, {14: BAD_DT}]),
    "pmoe_moe_loss": ([p1, p2, p3, p4, p5, p6, 0.75, 0.25, p7, p8, p9, p10, p11, p12, 4, 4, 0, None], [{15: 0}, {15: 65}]),
    # ---- punet.hip
    "pmoe_maxpool2s2_fwd": ([p1, p2, 2, 8, 8, 64, 64, 0, 0, None], [{3: 1}, {4: 1}, {2: 0}, {5: 60}, {8: 1, 5: 62}, {8: BAD_DT}] + _window(6, 7)),
    "pmoe_pixel_shuffle2": ([p1, p2, 2, 8, 8, 64, 256, 64, 0, 0, None], [{5: 60}, {6: 260}, {6: 128}, {9: BAD_DT}] + _window(7, 8)),
    "pmoe_copy_window": _window_copy,
    "pmoe_action_head_fwd": ([p1, 8, p2, 4, p3, p4, 4, 0, None], [{6: 0}, {1: 1}, {3: 0}, {7: BAD_DT}]),
    "pmoe_action_head_bwd": ([p1, p2, p3, p4, 8, p5, 4, 4, 0, None], [{7: 0}, {4: 1}, {6: 0}, {8: BAD_DT}]),
    "pmoe_action_loss": ([p1, p2, p3, p4, 0.75, 0.25, p5, p6, p7, 4, None], [{9: 0}, {3: None}, {8: None}]),
    "pmoe_blend_fwd": ([p1, p2, p3, p4, p5, p6, p7, 4, None], [{7: 0}]),
    "pmoe_blend_bwd": ([p1, p2, p3, p4, p5, p6, p7, p8, p9, p10, p11, 4, None], [{11: 0}]),
    "pmoe_history_push": ([p1, p2, 2, 4, 192, 1, p3, 3, 8, 0, None],
                          _nulls(0, 1) + [{2: 0}, {2: BIG}, {3: 0}, {4: 0}, {5: BAD_DT}, {5: 0}, {7: 0}, {8: 2}, {4: 193}, {6: p3 + 8},
                                          {9: 1, 8: 6}, {9: BAD_DT}, {8: 12}]),
    "pmoe_mixture_draw": ([p1, p2, p3, p4, p5, p6, p7, p8, p9, p10, p11, 4, 4, None],
                          _nulls(0, 1, 2, 3, 4, 6, 7, 8, 9, 10) + [{11: 0}, {12: 0}, {3: p4 + 4}]),
    # ---- stage1.hip
    "pmoe_maxpool2s2_bwd": ([p1, 64, 0, p2, p3, 64, 0, p4, 2, 8, 8, 64, 0, None],
                            [{8: 0}, {9: 0}, {10: 0}, {9: 7}, {10: 7}, {11: 60}, {12: BAD_DT}] + _window(1, 2) + _window(5, 6)),
    "pmoe_pixel_unshuffle2": ([p1, 64, 0, p2, 256, 2, 8, 8, 64, 0, None],
                              [{5: 0}, {6: 0}, {7: 0}, {8: 60}, {4: 260}, {4: 128}, {9: BAD_DT}] + _window(1, 2)),
    "pmoe_add_window": _window_copy,
    "pmoe_cat_windows": (["host8", 2, 32, 32, 0, p1, 64, 64, 16, 0, None],
                         [{0: None}, {1: 0}, {1: 9}, {2: 0}, {4: -1}, {4: 8}, {8: -1}, {7: 128}, {2: 48, 3: 64},
                          {7: 60, 2: 30}, {6: 68}, {9: BAD_DT}]),
    "pmoe_nhwc_to_nchw": ([p1, 64, 0, p2, 2, 64, 23, 0, None], [{4: 0}, {5: 0}, {6: 0}, {2: 48}, {6: 2048, 1: 4096}, {5: 1 << 40}, {7: BAD_DT}]),
    "pmoe_seg_loss_rows": ([2, 8, 8], [{0: 0}, {1: 0}, {2: 0}]),
    "pmoe_seg_loss_cp": ([23], [{0: 1}, {0: 33}]),
    "pmoe_seg_loss_fwd": ([p1, p2, 2, 3, 23, 8, 8, 0, 0.5, 0.5, 0.25, 0.75, p3, p4, p5, p6, p7, None],
                          [{2: 0}, {3: 0}, {4: 1}, {4: 33}, {5: 0}, {6: 0}, {7: -1}, {7: 3}] + _nulls(13, 16, 12, 14, 15)),
    "pmoe_seg_loss_bwd": ([p1, p2, p3, p4, p5, p6, 2, 3, 23, 8, 8, 0, None],
                          [{6: 0}, {7: 0}, {8: 1}, {8: 33}, {9: 0}, {10: 0}, {11: -1}, {11: 3}] + _nulls(5, 2, 3)),
    # ---- stage0.hip
    "pmoe_dice_score": ([p1, p2, 2, 23, 64, 0.5, p3, p4, None], _nulls(0, 1, 6, 7) + [{2: 0}, {3: 0}, {3: 65}, {4: 0}]),
    "pmoe_dropout2d_table": ([p1, 2, 64, 0.5, 7, None], [{0: None}, {1: 0}, {2: 0}, {3: -0.5}, {3: 1.5}]),
    "pmoe_channel_scale": ([p1, 64, 0, p2, 2, 64, 64, 0, None],
                           _nulls(0, 3) + [{4: 0}, {5: 0}, {6: 0}, {2: -8}, {2: 8}, {6: 60}, {1: 68}, {1: 128, 2: 4},
                                           {7: 1, 6: 62}, {7: 1, 1: 66}, {7: 1, 1: 128, 2: 2}, {7: BAD_DT}]),
    # ---- optim.hip
    "pmoe_mt_grad_norm": ([p1, p2, p3, 4, 1.0, p4, p5, 1, None], _nulls(0, 5, 6) + [{3: 0}]),
    "pmoe_mt_adam": ([p1, p2, p3, 4, 0.5, 0.5, 0.5, 0.5, 0.0, 0, 1.0, 1.0, p4, None], [{3: 0}, {0: None}]),
    "pmoe_mt_adam_packs": ([p1, p2, p3, p4, p5, 4, 0.5, 0.5, 0.5, 0.5, 0.0, 0, 1.0, 1.0, p6, None], _packs),
    "pmoe_mt_rmsprop": ([p1, p2, p3, 4, 0.5, 0.5, 0.5, 0.0, 0.0, 0, p4, None], _nulls(0, 1, 2) + [{3: 0}]),
    "pmoe_mt_rmsprop_packs": ([p1, p2, p3, p4, p5, 4, 0.5, 0.5, 0.5, 0.0, 0.0, 0, p6, None], _packs),
    "pmoe_mt_swa_update": ([p1, p2, p3, 4, 0, None], [{3: 0}, {0: None}, {4: -1}]),
    # ---- preprocess.hip
    "pmoe_resample_u8_horizontal": ([p1, p2, 2, 8, 8, 0, 8, 3, 4, p3, p4, 3, None],
                                    _nulls(0, 1, 9, 10) + [{2: 0}, {6: 0}, {5: -1}, {5: 1}, {4: 0}, {8: 0}, {7: 0}, {11: 0}]),
    "pmoe_resample_u8_vertical_to_f32": _vertical,
    "pmoe_resample_u8_vertical_to_i64": _vertical,
    "pmoe_resample_u8_vertical_to_u8": _vertical,
    # ---- augment.hip (2^29 pixels per frame; 2^22 rows: more row blocks than grid.y holds)
    "pmoe_augment_point_to_u8": (_point[0], _point[1] + [{1: p1}]),
    "pmoe_augment_point_to_f32": _point,
    "pmoe_augment_blur_h": _blur,
    "pmoe_augment_blur_v": _blur,
}


def rows():
    """[[entry point, arguments], ...] of every refused call"""
    out = []
    for name, (good, changes) in CASES.items():
        for change in changes:
            args = list(good)
            for i, v in change.items():
                args[i] = v
            out.append([name, args])
    return out


def call(lib, name, args):
    """the return code of one call; the host arrays are built here and live until it returns"""
    host = {"host12": (C.c_void_p * 12)(*(0x100000 + 0x1000 * k for k in range(12))),
            "host8": (C.c_void_p * 8)(*(0x200000 + 0x1000 * k for k in range(8)))}
    return getattr(lib, name)(*(host[a] if isinstance(a, str) else a for a in args))


if __name__ == "__main__":
    import torch
    from pmoe_amd import hip
    assert not torch.cuda.is_available(), "record on a machine without a GPU: a call that is not refused would launch on made-up pointers"
    lib = hip.load()
    # without a GPU an accepted call fails in the runtime (a HIP error code > 0, or the row count of pmoe_seg_loss_rows / _cp):
    # every accepted argument list passes every check, so each row below trips exactly the check its change aims at
    for name, (good, _) in CASES.items():
        assert call(lib, name, good) > 0, (name, "accepted arguments are refused")
    table = [[name, args, call(lib, name, args)] for name, args in rows()]
    assert all(rc == hip.ERR_ARG for _, _, rc in table), [r for r in table if r[2] != hip.ERR_ARG]
    Path(sys.argv[1]).write_text("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in table) + "\n]\n")
    print("recorded", len(table), "refusals of", len(CASES), "entry points from", hip.lib_path())
