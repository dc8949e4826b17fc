"""Reference of the convolution entry points (pmoe_conv2d_igemm, pmoe_conv2d_wgrad / pmoe_conv2d_wgrad_fold, the weight packs and
pmoe_unpack_conv_wgrad), the input generators and the case table of tests/test_conv_cpu.py and tests/test_conv_gpu.py.

Pure torch on the CPU, float64.  One function per entry point, taking what the descriptor takes: NHWC activations with the experts
folded into the image index, channel windows (ld = the last dimension of the buffer, coff), the fused forms of include/pmoe_hip.h
that tests/bn_ref.py leaves out -- the statistics epilogue, PMOE_RES_INBN (BatchNorm + ReLU on load, on bn_ref.bn_apply),
PMOE_RES_DBN (masked gradient + the two reductions of the BatchNorm backward) and the bn_fused weight gradient (on
bn_ref.bn_bwd_apply) -- and the epilogue of the expert MLP layers: PMOE_ACT_ELU | TANH | SIGMOID, PMOE_RES_DELU | DTANH | DSIGMOID
and fused inverted dropout (mlp_epilogue, on tests/eca_head_ref.py's hash, keep_scale, activations and device-library allowances).
pmoe_mlp_wgrad (csrc/gemm_skinny.hip, mlp_wgrad_kernel) has its reference, cases and generator at the end of the file.

Three kinds of input (tests/test_conv_cpu.py checks on the CPU what the GPU tests assume of them):
  lattice  integers (BatchNorm coefficients: small dyadic numbers) with sum |x||w| < 2^24 per output element, so that every partial
           sum of a float32 accumulation is exact IN ANY ORDER and a kernel's accumulator IS the float64 one; wide enough that the
           bfloat16 output really rounds (inexactly and on exact ties).  What is left to a kernel is the order of its roundings:
           ROUNDING below.
  unit     {-1, 0, 1} with three quarters zeros: outputs below 256 (nothing rounds) and squared-output sums below 2^24, so that
           every fused statistic is exact too.
  dyadic   the cases that ask for an activation, its derivative or dropout, and only they: sparse small integers against
           weights and biases that are multiples of 1/64, so that the accumulator is still exact in any order (64 sum |x||w| <
           2^24) but the pre-activations spread over (-8, 8), where ELU, tanh and sigmoid are not saturated.  What is left to a
           kernel there is the device library's expm1f / tanhf / expf and the float32 operations behind them: mlp_epilogue
           returns that allowance next to the value, and zero wherever the value is a float32 product or nothing.
  select   the cases with e4m3 operands (flags f8 / a8), next to lattice and unit: every output channel has ONE non-zero weight,
           +-2^j at a random (tap, input channel), so an output element is +-2^j times the CONVERTED input at the shifted pixel
           (0 where the tap falls into the padding) -- one product, exact in bfloat16 in any order.  The inputs hold every e4m3
           value, every exact tie with its bfloat16 neighbours, values that underflow and values that saturate (select_values).
Continuous data stays in tests/test_ops_gpu.py for the K-long float32 SUMS only: a worst-case float32 bound over K = 4608 terms
is looser than bfloat16 rounding.

e4m3 operands (include/pmoe_hip.h, pmoe_conv_desc.w_fp8 / in_fp8; the policy: oracle/fp8_policy.py).  A launch with e4m3 weights
computes conv(qdq_act(x), qdq_weight(w)): products of two e4m3 factors are exact in float32 and every scale is a power of two, so
the accumulator is as exact as the bfloat16 one.  Integers up to 15 have four significant bits and a row of them scales to at most
448: the lattice and unit generators are FIXED POINTS of both quantisers (tests/test_conv_cpu.py asserts it), the reference of
such a launch is the reference itself, and an e4m3 kernel must store it bit for bit.
"""
import collections
import functools

import torch
import torch.nn.functional as F

from oracle import fp8_policy as P
from tests import bn_ref
from tests import eca_head_ref as H
from tests.stem_tail_ref import BF16, F32, F64, round_to

EPS24 = bn_ref.EPS24
RES_NONE, RES_ADD, RES_DRELU, RES_DELU, RES_DTANH, RES_DSIGMOID, RES_DBN, RES_INBN = range(8)          # include/pmoe_hip.h
ACT_NONE, ACT_RELU, ACT_ELU, ACT_TANH, ACT_SIGMOID = range(5)
KINDS = ("lattice", "unit")
DYADIC = "dyadic"                    # the one kind of the cases that ask for an MLP epilogue form (kinds_of)
SELECT = "select"                    # the third kind of the cases with e4m3 operands (kinds_of)
F8_FLAGS = {"f8", "a8"}              # e4m3 weights with bfloat16 input | e4m3 weights and e4m3 input bytes
IN_SCALE = P.IN_SCALE                # 16, the policy's; SCALE_FLAGS: the case that runs under another power of two
SCALE_FLAGS = {"sc32": 32.0}
DROP_P = 0.3
ACT_FLAGS = {"elu": ACT_ELU, "tanh": ACT_TANH, "sigmoid": ACT_SIGMOID}
DMODE_FLAGS = {"delu": RES_DELU, "dtanh": RES_DTANH, "dsigmoid": RES_DSIGMOID}
ACT_OF_DMODE = {RES_DRELU: ACT_RELU, RES_DELU: ACT_ELU, RES_DTANH: ACT_TANH, RES_DSIGMOID: ACT_SIGMOID}
DROP_FLAGS = ("drop", "dropL", "dropE")                                # SEED_OF below: seed 5, a seed above 2^32, edge_seed
MLP_FLAGS = set(ACT_FLAGS) | set(DMODE_FLAGS) | set(DROP_FLAGS)


def r16(c):
    return (c + 15) // 16 * 16


def r64(c):
    return (c + 63) // 64 * 64


def out_size(h, ks, stride, pad):
    return (h + 2 * pad - ks) // stride + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the order of roundings of the stored value, per plan code (include/pmoe_hip.h lists the codes)
#
#   "once"    stored = round(epilogue(acc + bias, res))            the accumulator meets bias and side input in float32
#   "staged"  stored = round(epilogue(round(acc + bias), res))     the accumulator is staged as bfloat16 first
#
# The two differ only where something is ADDED to the accumulator after the staging (PMOE_RES_ADD): a mask (PMOE_RES_DRELU,
# PMOE_RES_DBN) selects between the value and zero and a ReLU keeps or clears it, whichever side of the rounding they sit on; bias
# is always added before the first rounding.  float32 storage rounds nothing on the lattice.  Each entry: the order of a
# PMOE_RES_ADD launch without bias / activation, the order with one of them (None: the kernel takes no such launch), and the code
# that decides it.
Order = collections.namedtuple("Order", "add add_bias_act where")
_TILE = Order("once", "once", "conv_igemm.hip conv_igemm_body: f32 staging, `v[i] += rv[i]` before pack16<T>")
_RES = Order("staged", None, "conv_res.hip: `(bf16)acc` into the staging region, then unpack16 + `v[i] += rv[i]` + pack16")
_DMA = Order("staged", "once", "conv_dma_epilogue.inc: fast_epi (add_fast under DMA_ZPRE) stages bf16; bias / act take the two-phase f32 path")
_DMA2P = Order("once", "once", "conv_dma_epilogue.inc: no DMA_ZPRE in conv3x3s2_dma_kernel, RES_ADD takes the two-phase f32 path")
_NOADD = Order(None, None, "takes no side input")
# e4m3 operands on the generic tile: the same tail, `v[i] *= osc[i]` (a power of two: exact), then bias, then the residual, all in
# float32 (conv_igemm.hip:327-338).  8507 (conv_dma.hip conv_dma_f8_plan: res_mode != PMOE_RES_NONE is refused) takes no side
# input; its one-phase read-out applies the power-of-two out_scale to the bfloat16-staged accumulator, which is the rounding of the
# scaled accumulator (conv_dma_epilogue.inc:69-73).
_TILE8 = Order("once", "once", "conv_igemm.hip:327-338: `v[i] *= osc[i]`, `v[i] += bias[i]`, `v[i] += rv[i]` in f32 before pack16<T>")
ROUNDING = {
    **{c: _TILE for c in (522, 541, 542, 622, 641, 642, 722, 741, 742, 2007)},                  # conv_igemm_kernel / _lite_kernel
    **{4000 + c: _TILE for c in (522, 541, 542, 622, 641, 642, 722, 741, 742, 2007)},           # ... as parity-class launches
    **{8000 + c: _TILE8 for c in (622, 641, 642, 722, 741, 742, 2007)},                         # ... with e4m3 operands (64 | 128-channel chunks)
    8507: _NOADD,                                                                               # conv3x3_dma_f8_kernel
    3000: _TILE,                                        # gemm_skinny_kernel<4>: its four f32 partial tiles and the bias meet in registers, the same tail
    1005: _RES, 1007: _RES,                                                                     # conv3x3_res_kernel
    1107: _RES, 1117: _NOADD,                                                                   # conv3x3_resdma_kernel
    1207: _NOADD, 1217: _NOADD, 1227: _RES, 1247: _NOADD, 1257: _NOADD, 1267: _NOADD,          # conv3x3_respipe_kernel<b, m>
    1316: _NOADD,                                                                               # conv3x3_c16_kernel
    **{c: _NOADD for c in (1402, 1404, 1412, 1414, 1452, 1454, 1462, 1464)},                    # conv1x1_direct_kernel
    5007: _DMA, 5017: _DMA,                                                                     # conv3x3_dma_kernel<MF16>
    5027: _NOADD, 5037: _NOADD, 5047: _NOADD, 5057: _NOADD, 5067: _NOADD,                      # producer wave / persistent: plain launches
    5207: _DMA2P, 9207: _DMA2P,                                                                 # conv3x3s2_dma_kernel<CLS>
}


def rounding_of(code, res_mode, bias, act):
    """the order of roundings the kernel behind ``code`` implements for this launch"""
    if res_mode != RES_ADD:
        return "once"
    o = ROUNDING[code]
    order = o.add_bias_act if (bias or act != ACT_NONE) else o.add
    assert order is not None, f"plan code {code} is not expected to take this PMOE_RES_ADD launch"
    return order


# The weight-gradient workspace dw_ws [E | N][ks*ks][coutp][cinp]: its pad rows (>= cout) and pad columns (>= cin) are ZEROS, not
# untouched -- every element is stored (include/pmoe_hip.h; conv_wgrad.hip's flush writes whole channel tiles and zero-fills past
# CinP's real columns).  With `grads` set the workspace is scratch and only `grads` is specified.
#
# Longest chain of sequential float32 additions behind one statistics ROW, read from the kernels (as bn_ref.chain_stream does for
# the stand-alone passes).  T = the tiles one workgroup walks = ceil(tiles per expert / rows per expert).
#   conv_igemm.hip:312,370,393,411   one row per 256 | 128-pixel tile: BMH / PROWS <= 16 read-outs per thread, <= 3 xor-shuffles,
#                                    <= 8 waves through LDS                                                  L = 16 + 3 + 8
#                                    (the same body with e4m3 operands, 8000 + code: the statistics read the packed bfloat16
#                                    back, conv_igemm.hip:364-370; <4, 2> = 742 | 8742: 256 / 32 = 8 read-outs, 2 shuffles)
#   conv_dma_epilogue.inc:189,257,274 one row per tile: BM / PROWS = 8 (4: 64-cout tiles), 2 (3) shuffles, 8 waves    L = 8 + 3 + 8
#                                    (8507, conv3x3_dma_f8_kernel, includes it under DMA_OSCALE, conv_dma.hip:1173-1175:
#                                    BM / PROWS = 256 / 32 = 8 read-outs, shuffles over 16 and 32 lanes, 8 waves)
#   conv_res.hip:214,242,261          conv3x3_res_kernel: 8 per tile, 3 shuffles, 8 waves                     L = 8 T + 11
#   conv_res.hip:506,541,568          conv3x3_resdma_kernel: 4 per tile                                       L = 4 T + 11
#   conv_res.hip:825,841,983,997      conv3x3_respipe_kernel: 2 per tile, 5 shuffles, 4 waves                 L = 2 T + 9
#   conv_c16.hip:120,131,179          a wave takes every 4th tile, 4 pixels each; 4 waves x 8 lane groups    L = 4 ceil(T / 4) + 32
#   conv_c1x1.hip:154,174,217         every 4th tile, PASSES <= 8 pixels each; 4 waves x PPP <= 8 groups      L = 8 ceil(T / 4) + 32
def chain_stats(code, tiles_per_expert, rows_per_expert):
    T = bn_ref.cdiv(tiles_per_expert, rows_per_expert)
    if code in (1005, 1007):
        return 8 * T + 11
    if code in (1107, 1117):
        return 4 * T + 11
    if 1200 <= code < 1300:
        return 2 * T + 9
    if code == 1316:
        return 4 * bn_ref.cdiv(T, 4) + 32
    if 1400 <= code < 1500:
        return 8 * bn_ref.cdiv(T, 4) + 32
    if 5000 <= code < 6000 or code == 8507:
        return 19
    return 27


def tiles_per_expert(code, ipe, ho, wo):
    """tiles of one expert as the kernel behind ``code`` cuts them: kernels.h pixel_tile (256 pixels, rows of <= 32), rows of 32
    pixels (conv_c16.hip) or runs of 32 pixels (conv_c1x1.hip); 1: a kernel with one statistics row per tile"""
    if code == 1316:
        return ipe * ho * bn_ref.cdiv(wo, 32)
    if 1400 <= code < 1500:
        return bn_ref.cdiv(ipe * ho * wo, 32)
    if 1000 <= code < 1300:
        clog = lambda v: (v - 1).bit_length()
        ltw = min(clog(wo), 5)
        lth = min(clog(ho), 8 - ltw)
        tn = 256 >> (ltw + lth)
        return bn_ref.cdiv(ipe, tn) * bn_ref.cdiv(ho, 1 << lth) * bn_ref.cdiv(wo, 1 << ltw)
    return 1


# ---------------------------------------------------------------------------------------------------------------------------------
# weight packs (csrc/heads.hip): permutations and one rounding

def pack_weights(ws, coutp, cinp, dtype, cinp2=None, coutp2=None):
    """pack_w_kernel: ws [E, cout, cin, ks, ks] -> fwd [E, coutp, ks*ks, cinp] and (cinp2 given) dgrd [E, cinp2, ks*ks, coutp2] with
    dgrd[e, ci, taps - 1 - t, co] = ws[e, co, ci, t]; zero padded, rounded to the storage type"""
    E, cout, cin, ks, _ = ws.shape
    w = round_to(ws.reshape(E, cout, cin, ks * ks), dtype)
    fwd = torch.zeros(E, coutp, ks * ks, cinp, dtype=F64)
    fwd[:, :cout, :, :cin] = w.permute(0, 1, 3, 2)
    if cinp2 is None:
        return fwd
    dgrd = torch.zeros(E, cinp2, ks * ks, coutp2, dtype=F64)
    dgrd[:, :cin, :, :cout] = w.flip(3).permute(0, 2, 3, 1)
    return fwd, dgrd


def pack_weights_scaled(ws, scale, shift, mean, coutp, cinp, dtype):
    """pack_w_scaled_kernel: fwd = round(ws * scale[e, co]) and bias [E, coutp] = shift - mean * scale (float32, one rounding of
    the product and one of the difference; exact on the lattice)"""
    E, cout = ws.shape[:2]
    fwd = pack_weights(ws * scale[:, :, None, None, None], coutp, cinp, dtype)
    bias = torch.zeros(E, coutp, dtype=F64)
    bias[:, :cout] = shift - mean * scale
    return fwd, bias


def pack_weights_gated(ws, gate, ipe, coutp, cinp, dtype, cinp2, coutp2):
    """pack_w_gated_kernel: per IMAGE packs of ws[n // ipe] * gate[n, ci]; gate [N, >= cin]"""
    cin = ws.shape[2]
    wn = ws.repeat_interleave(ipe, 0) * gate[:, None, :cin, None, None]
    return pack_weights(wn, coutp, cinp, dtype, cinp2, coutp2)


def unpack_wgrad(dw_ws, cout, cin, ks):
    """unpack_wgrad_kernel: dw_ws [E, ks*ks, coutp, cinp] -> grads [E, cout, cin, ks, ks]"""
    E = dw_ws.shape[0]
    return dw_ws[:, :, :cout, :cin].permute(0, 2, 3, 1).reshape(E, cout, cin, ks, ks).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# pmoe_conv2d_igemm

def _padded_source(xw, ks, stride, pad, ho, wo, dilate):
    """[Nin, H, W, C] -> NCHW source of a plain strided correlation that yields [ho, wo]: zero-upsampled by 2 (dilate), `pad`
    zeros before, whatever the output extent needs after"""
    x = xw.permute(0, 3, 1, 2)
    if dilate:
        n, c, h, w = x.shape
        u = x.new_zeros(n, c, 2 * h - 1, 2 * w - 1)
        u[:, :, ::2, ::2] = x
        x = u
    h, w = x.shape[2:]
    pb, pr = (ho - 1) * stride + ks - h - pad, (wo - 1) * stride + ks - w - pad
    return F.pad(x, (pad, max(pr, 0), pad, max(pb, 0)))


def conv_acc(xw, w, *, ipe, in_shared, stride, pad, ho, wo, dilate=False, dtype=F64, taps=False, shift_tap=False):
    """the accumulator: xw [Nin, H, W, cin] (the channel window), w [E, cout, cin, ks, ks] -> [N, ho, wo, cout], evaluated in
    ``dtype``.  taps: a tap-by-tap loop (another summation order than F.conv2d's).  shift_tap (a mutant): the left tap of the
    middle filter row reads the image's first column where it should read the zero border"""
    E, cout, _, ks, _ = w.shape
    x = _padded_source(xw.to(dtype), ks, stride, pad, ho, wo, dilate)
    xm = x
    if shift_tap and pad > 0:
        xm = x.clone()
        xm[:, :, :, pad - 1] = x[:, :, :, pad]
    outs = []
    for e in range(E):
        xe = x if in_shared else x[e * ipe:(e + 1) * ipe]
        we = w[e].to(dtype)
        if not taps and not shift_tap:
            outs.append(F.conv2d(xe, we, stride=stride)[:, :, :ho, :wo])
            continue
        o = torch.zeros(xe.shape[0], cout, ho, wo, dtype=dtype)
        for ky in reversed(range(ks)):
            for kx in range(ks):
                src = (xm if in_shared else xm[e * ipe:(e + 1) * ipe]) if (ky, kx) == (ks // 2, 0) else xe
                v = src[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
                o = o + torch.einsum("nchw,oc->nohw", v, we[:, :, ky, kx])
        outs.append(o)
    return torch.cat(outs).permute(0, 2, 3, 1).contiguous()


def _per_image(coef, bn_ipe):
    """[Ebn, C] -> [N, 1, 1, C]"""
    return coef.repeat_interleave(bn_ipe, 0)[:, None, None, :]


def _f32(t):
    """one float32 rounding"""
    return round_to(t, F32)


_M64 = (1 << 64) - 1


def edge_seed(idx, drop_p=DROP_P):
    """a seed under which hash_uniform(seed, idx) == float32(drop_p) EXACTLY -- the one element that tells the keep test `>=` from
    `>`.  float32(0.3) is a multiple of 2^-24, and the mix of csrc/common.h is a bijection of 64-bit words: run it backwards from
    a word whose top 24 bits are that multiple."""
    def unxorshift(y, s):
        x = y
        for _ in range(64 // s + 1):
            x = y ^ (x >> s)
        return x
    top = int(torch.tensor(drop_p, dtype=F32).to(F64).item() * 16777216.0)
    z = unxorshift((top << 40) | 0x5A5A5A5A5A, 31)
    z = unxorshift(z * pow(0x94D049BB133111EB, -1, 1 << 64) & _M64, 27)
    z = unxorshift(z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64) & _M64, 30)
    return (z - idx * 0x9E3779B97F4A7C15) & _M64


EDGE_INDEX = 11
SEED_OF = {"drop": H.SEEDS[0], "dropL": H.SEEDS[1], "dropE": edge_seed(EDGE_INDEX)}

# deliberately wrong variants of the reference (``mut``); tests/test_conv_cpu.py proves that the cases tell each from the reference
MUTANTS = ("kslice",              # the last k-slice of 16 input channels dropped
           "tapshift",            # one tap reads the image's first column in place of the zero border
           "bias_late",           # the bias added after a staging rounding
           "drop_ld",             # the dropout index computed with out_ld in place of Cout
           "drop_off1",           # ... off by one
           "keep_gt",             # kept iff hash > p
           "dmode_noscale",       # keep_scale left out of a D-mode
           "dmode_unscaled")      # the saved output used unscaled in f'


def _op(value, err):
    """the error bound of one float32 operation whose exact result is ``value`` and whose operands carry ``err`` into it: nothing
    new where the operands are exact and the result is a float32 value, else one rounding of the result"""
    err = err + torch.zeros_like(value)
    return err + torch.where((err > 0) | (value != _f32(value)), EPS24 * value.abs(), torch.zeros_like(value))


def mlp_epilogue(v, rw, *, res_mode, act, drop_p, seed, out_ld=0, mut=""):
    """The tail the three epilogue copies share (csrc/gemm_skinny.hip:136-166, conv_igemm.hip:333-363,
    conv_dma_epilogue.inc:90-115): v [N, Ho, Wo, cout] = acc + bias, exact; rw = the residual window.  Residual mode, then
    activation, then dropout.  -> value (float64; where ``allow`` is zero, the float32 value itself), allow (the allowance on
    the float32 value), keep (the dropout mask), undropped (the value before the dropout).

    EXACT (allow = 0): no activation and ReLU, with or without dropout; PMOE_RES_DRELU with keep_scale; ELU and its derivative
    on the positive branch -- all a float32 product with the float32 keep_scale, or nothing: round_f32(v * keep_scale).
    Allowances, in units of 2^-24 = one float32 rounding of the magnitude named (H.ULP = 2 units):
      ELU, v <= 0   T_EXPM1 ULP |y|                        tanh   T_TANH ULP |y|
      sigmoid       T_EXP ULP y (1 - y) + 2 |y|            (1 + e and the division, as eca_head_ref.act_fwd)
      ... with dropout: times keep_scale, + 1 |y keep_scale| for the product `v[i] * keep_scale`
    D-modes, u = rv * (1 / keep_scale), result dy f'(u) keep_scale: the error bound is carried operation by operation (_op) --
    an operation whose operands are exact and whose exact result is a float32 value adds nothing, any other adds one unit of
    its result on top of what its operands carry through it.  So a chain that float32 evaluates exactly (a bfloat16 saved
    output without dropout: u = rv, u^2 has 16 bits, and the dyadic dy times a short f' often fits 24) must come out EXACT,
    bfloat16 ties included, and only what really rounds gets an allowance:
      `1.f / keep_scale`, `rv * (...)`     with dropout: u carries 2 units of |u|
      DELU, u <= 0   `y + 1.f`, `v * d`           DSIGMOID   `1.f - y`, `y * (...)`, `v * d`
      DTANH          `y * y`, `1.f - (...)`, `v * d`: the compiler may contract the first two into one rounding of 1 - u^2,
                     which the two-step bound covers (it is never below one unit of the result)
      `* keep_scale` with dropout
    A saved output of exactly 0 under dropout counts as dropped."""
    zero = torch.zeros((), dtype=F64)
    allow = torch.zeros_like(v)
    ks = H.keep_scale(drop_p, F64)                                      # float32(1 / (1 - float32(p))), or 1
    drop = drop_p > 0
    if res_mode == RES_ADD:
        v = v + rw
    elif res_mode == RES_DRELU:
        v = torch.where(rw > 0, v if mut == "dmode_noscale" else _f32(v * ks), zero)
    elif res_mode in (RES_DELU, RES_DTANH, RES_DSIGMOID):
        assert act == ACT_NONE, "a derivative mode and an activation do not combine in the engine"
        sc = 1.0 if mut == "dmode_noscale" else ks
        u, eu = rw, torch.zeros_like(rw)
        if drop and mut != "dmode_unscaled":
            u = rw / ks
            eu = _op(u, rw.abs() * _op(1 / ks, 0 * ks))
        if res_mode == RES_DELU:
            dv = u + 1
            ed = _op(dv, eu)
        elif res_mode == RES_DTANH:
            dv = 1 - u * u
            ed = _op(dv, _op(u * u, 2 * u.abs() * eu))
        else:
            t = 1 - u
            et = _op(t, eu)
            dv = u * t
            ed = _op(dv, t.abs() * eu + u.abs() * et)
        raw = v * dv
        al = _op(raw, v.abs() * ed)
        if drop and mut != "dmode_noscale":
            raw = raw * sc
            al = _op(raw, sc * al)
        if res_mode == RES_DELU:
            raw, al = torch.where(u > 0, _f32(v * sc), raw), torch.where(u > 0, zero, al)
        dropped = (rw == 0) & drop
        v, allow = torch.where(dropped, zero, raw), torch.where(dropped, zero, al)
    if act == ACT_RELU:
        v = v.clamp_min(0)
    elif act != ACT_NONE:
        assert res_mode in (RES_NONE, RES_ADD)
        y = H.act_apply(act, v)
        allow = {ACT_ELU: H.T_EXPM1 * H.ULP * torch.where(v > 0, zero, y.abs()), ACT_TANH: H.T_TANH * H.ULP * y.abs(),
                 ACT_SIGMOID: H.T_EXP * H.ULP * y * (1 - y) + 2 * EPS24 * y.abs()}[act]
        v = y
    undropped, keep = v, torch.ones_like(v, dtype=torch.bool)
    if drop and res_mode < RES_DRELU:
        # element (opix, c) of the dense NHWC output draws hash_uniform(seed, opix * Cout + c)
        cout = v.shape[-1]
        ld = out_ld if mut == "drop_ld" else cout
        idx = (torch.arange(v.numel() // cout)[:, None] * ld + torch.arange(cout)).reshape(v.shape) + (mut == "drop_off1")
        u = H.hash_uniform(seed, int(idx.max()) + 1)[idx]
        p = torch.tensor(drop_p, dtype=F32).to(F64)
        keep = (u > p) if mut == "keep_gt" else (u >= p)
        scaled = torch.where(allow > 0, v * ks, _f32(v * ks))
        al = torch.where(allow > 0, allow * ks + EPS24 * (v * ks).abs(), zero)
        v, allow = torch.where(keep, scaled, zero), torch.where(keep, al, zero)
    return {"value": v, "allow": allow, "keep": keep, "undropped": undropped}


def conv2d(inp, w, out_init, *, cin, cout, ipe, ks, stride, pad, dtype, in_shared=False, in_coff=0, out_coff=0, dilate=False,
           bias=None, res=None, res_coff=0, res_mode=RES_NONE, act=ACT_NONE, bn_coef=None, bn_ipe=0, shuffle_c=0, stats=False,
           rounding="once", drop_p=0.0, seed=0, mut=""):
    """pmoe_conv2d_igemm.  inp [Nin, H, W, in_ld], w [E, cout, cin, ks, ks] (the launch's own orientation: a data gradient passes
    the flipped, transposed filter), out_init [N, Ho, Wo, out_ld] = the output buffer before the launch ([N, 2 Ho, 2 Wo, out_ld]
    with shuffle_c), bias [E, cout], res [N, Ho, Wo, res_ld], bn_coef [4, N / bn_ipe, C] = mean, invstd, gamma * invstd, beta.
    -> acc (the exact accumulator), stored (the rounded window), out (the whole buffer after the launch), and with ``stats`` the
    per-expert totals ``sums`` [E, 2, cout] with ``sums_abs`` (the sums of the absolute values of the same terms).
    act / res_mode beyond ReLU / DRELU and drop_p, seed: the MLP forms of mlp_epilogue, whose ``allow`` (the allowance on the
    float32 value of the window; zero = the stored value is exact), ``keep`` and ``undropped`` come back too.  ``mut``: MUTANTS"""
    E = w.shape[0]
    n = out_init.shape[0]
    ho, wo = out_init.shape[1:3]
    if shuffle_c:
        ho, wo = ho // 2, wo // 2
    xw = inp[..., in_coff:in_coff + cin]
    if res_mode == RES_INBN:
        # the operand is what pmoe_bn_apply(relu = 1) would have stored; the zero padding applies to the activation, not to z
        mean, scale, shift = bn_coef[0], bn_coef[2], bn_coef[3]
        xw = bn_ref.bn_apply(xw, None, scale, shift, mean, mean.shape[0], True, dtype)["y"]
    assert not torch.isnan(xw).any()
    if mut == "kslice":
        xw = torch.cat([xw[..., :-16], torch.zeros_like(xw[..., -16:])], -1)
    acc = conv_acc(xw, w, ipe=ipe, in_shared=in_shared, stride=stride, pad=pad, ho=ho, wo=wo, dilate=dilate,
                   shift_tap=mut == "tapshift")
    if mut == "bias_late":
        acc = round_to(acc, dtype)
    v = acc if bias is None else acc + bias.repeat_interleave(ipe, 0)[:, None, None, :]
    if rounding == "staged":
        v = round_to(v, dtype)
    xhat = None
    rw = res[..., res_coff:res_coff + cout] if res_mode not in (RES_NONE, RES_INBN) else None
    if res_mode == RES_DBN:
        mean, invstd, scale, shift = (_per_image(c, bn_ipe or ipe) for c in bn_coef)
        d = rw - mean
        v = torch.where(d * scale + shift > 0, v, torch.zeros((), dtype=F64))
        xhat = d * invstd
    ep = mlp_epilogue(v, rw, res_mode=RES_NONE if res_mode in (RES_DBN, RES_INBN) else res_mode, act=act, drop_p=drop_p, seed=seed,
                      out_ld=out_init.shape[-1], mut=mut)
    v, allow = ep["value"], ep["allow"]
    stored = round_to(v, dtype)
    out = out_init.clone()
    if shuffle_c:
        c = shuffle_c
        for q in range(4):
            out[:, q >> 1::2, q & 1::2, out_coff:out_coff + c] = stored[..., q * c:(q + 1) * c]
    else:
        out[..., out_coff:out_coff + cout] = stored
    r = {"acc": acc, "pre": v, "stored": stored, "out": out, "allow": allow, "keep": ep["keep"], "undropped": ep["undropped"]}
    if stats:
        t1 = stored.reshape(E, -1, cout)
        t2 = t1 * (t1 if xhat is None else xhat.reshape(E, -1, cout))
        r["sums"] = torch.stack([t1.sum(1), t2.sum(1)], 1)
        r["sums_abs"] = torch.stack([t1.abs().sum(1), t2.abs().sum(1)], 1)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# pmoe_conv2d_wgrad / pmoe_conv2d_wgrad_fold

def wgrad(x, dy, *, cin, cout, cinp, coutp, ipe, ks, stride, pad, dtype, x_shared=False, x_coff=0, dy_coff=0, per_image=False,
          bn=None, evaluate=F64):
    """x [Nin, H, W, x_ld], dy [N, Ho, Wo, dy_ld] -> dw_ws [E | N (per_image), ks*ks, coutp, cinp] (pad rows and columns: zeros,
    every element is stored) and, without per_image, grads [E, cout, cin, ks, ks].
    bn = (z [N, Ho, Wo, z_ld], coef [4, E, cout], c1 [E, cout], c2 [E, cout]): ``dy`` is g and the gradient that meets x is
    dz = bn_ref.bn_bwd_apply(g, relu = 0), rounded to the storage type as that kernel stores it"""
    n, ho, wo = dy.shape[:3]
    E = n // ipe
    g = dy[..., dy_coff:dy_coff + cout]
    if bn is not None:
        z, coef, c1, c2 = bn
        g = bn_ref.bn_bwd_apply(g, None, z[..., :cout], coef[0], coef[1], coef[2], coef[3], c1, c2, E, False, dtype)["dx"]
    assert not torch.isnan(g).any()
    xs = _padded_source(x[..., x_coff:x_coff + cin].to(evaluate), ks, stride, pad, ho, wo, False)
    g = g.to(evaluate)
    per = torch.zeros(n, ks * ks, coutp, cinp, dtype=evaluate)
    idx = torch.arange(n) % ipe if x_shared else torch.arange(n)
    for ky in range(ks):
        for kx in range(ks):
            v = xs[idx][:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
            per[:, ky * ks + kx, :cout, :cin] = torch.einsum("nhwo,nchw->noc", g, v)
    r = {"dz": g, "per_image": per}
    if per_image:
        r["dw_ws"] = per
    else:
        r["dw_ws"] = per.reshape(E, ipe, ks * ks, coutp, cinp).sum(1)
        r["grads"] = unpack_wgrad(r["dw_ws"], cout, cin, ks)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
#
# (E, ipe, cin, cout, H, W, ks, stride, dtype, request, switches) -> (forward, data gradient, weight gradient) plan codes.
# ``request``: what each of the three launches asks for, "f:<flags> d:<flags> w:<flags>" (a launch without a section is not run and
# its code is None); flags joined by "+":
#   f:  stats | bias | relu | add (PMOE_RES_ADD from its own buffer) | addin (res == out) | drelu | inbn | shuf (shuffle_c =
#       cout / 4) | shared (in_shared)
#   d:  add | addin (PMOE_RES_ADD with res == out: accumulated in place) | drelu | dbn | bias | pimg (the launch runs per image:
#       ipe = 1 under BatchNorm sets of ipe images, the ECA-gated stem)     -- stride 2: the zero-dilated form (`dilate`)
#   w:  pimg (per_image) | bn (bn_fused) | shared (x_shared)
#   win (any launch): input, output and residual are channel windows of wider rows, NaN outside
#   f:  f8 (e4m3 weight bytes with their out_scale, bfloat16 input converted by the loader) | a8 (e4m3 input bytes too: 0x7f, the
#       e4m3 NaN, outside the window), under in_scale 16 or sc32 (in_scale 32); such a case also runs on the select kind
#   the MLP forms (MLP_FLAGS; a case that names one runs on the dyadic kind alone):
#   f:  elu | tanh | sigmoid, drop | dropL | dropE (drop_p = 0.3 under seed 5 | a seed above 2^32 | edge_seed: one element's
#       hash EQUALS p)        d:  delu | dtanh | dsigmoid (and drelu), + drop: the saved output was dropped out under that seed
# ``switches``: environment values the launch is planned and run under.
Case = collections.namedtuple("Case", "E ipe cin cout H W ks stride dtype request switches codes")

MF16 = (("PMOE_DMA_MF16", "1"),)
NOSTREAM = (("PMOE_DMA_STREAM", "0"),)
DMA_ONE_TILE = (("PMOE_DMA_STREAM", "0"), ("PMOE_DMA_PRODUCER", "0"))
DMA_PRODUCER = (("PMOE_DMA_STREAM", "0"), ("PMOE_DMA_PRODUCER", "2"))


def _case(E, ipe, cin, cout, H, W, ks, stride, dtype, request, codes, switches=()):
    return Case(E, ipe, cin, cout, H, W, ks, stride, dtype, request, tuple(switches), codes)


CASES = [
    # ---- conv_igemm_kernel<T, LOG_RB, WM, WN> (the generic tile): every instantiation, both dtypes, forward with statistics (so
    #      that the skinny GEMM declines), data gradients stride 1 and 2 (parity classes, odd sides), the in-place 1x1 form
    _case(2, 3, 16, 16, 7, 5, 1, 1, BF16, "f:stats+win d:add w:", (541, 3000, 6106)),
    _case(2, 2, 16, 128, 7, 9, 1, 2, BF16, "f:stats d:addin w:win", (522, 741, 6106)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f:stats+bias d:add+win w:", (641, 4741, 6910)),
    _case(2, 1, 32, 128, 8, 8, 3, 1, BF16, "f:stats+add d: w:", (622, 3000, 6910)),
    _case(1, 2, 64, 48, 13, 9, 3, 2, BF16, "f:stats+relu+bias+win d:addin w:", (641, 4541, 6910)),
    _case(1, 2, 64, 128, 9, 9, 3, 2, BF16, "f:stats d: w:shared", (722, 4741, 6910)),
    _case(1, 2, 128, 64, 7, 7, 3, 2, BF16, "f:stats d:drelu w:", (641, 4722, 6906)),
    _case(2, 3, 64, 32, 9, 9, 3, 1, BF16, "f:stats+relu+bias d: w:", (741, 3000, None)),
    _case(1, 2, 128, 32, 13, 9, 3, 2, BF16, "f: d:add w:", (None, 4622, None)),
    _case(1, 2, 128, 16, 13, 9, 3, 2, BF16, "f: d:addin w:", (None, 4522, None)),
    _case(1, 2, 64, 32, 13, 9, 3, 2, BF16, "f: d:drelu+win w:", (None, 4641, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f:stats+win d:add w:", (641, 4641, 6912)),
    _case(1, 2, 16, 128, 9, 7, 1, 2, F32, "f:bias+relu d:addin w:", (622, 741, 6112)),
    _case(2, 2, 32, 32, 8, 8, 3, 1, F32, "f:stats+add d:drelu+win w:win", (741, 741, 6920)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f:stats d:bias w:", (722, 4741, 6912)),
    _case(1, 2, 128, 32, 7, 7, 3, 2, F32, "f:shared+bias d:add w:shared", (641, 4722, 6912)),
    _case(1, 2, 128, 8, 9, 7, 3, 2, F32, "f: d:addin w:", (None, 4522, None)),
    _case(1, 2, 128, 16, 9, 7, 3, 2, F32, "f: d:plain w:", (None, 4622, None)),
    _case(1, 2, 16, 8, 9, 7, 3, 2, F32, "f:stats d:add w:", (641, 4541, 6920)),
    _case(1, 1, 16, 128, 64, 66, 1, 1, BF16, "f:stats+add+win d:drelu w:", (542, 741, 6106)),
    _case(1, 1, 32, 128, 64, 66, 1, 1, BF16, "f:bias+relu d: w:", (642, None, None)),
    _case(1, 1, 64, 128, 64, 66, 1, 1, BF16, "f:add+stats d: w:", (2007, None, None), (("PMOE_CONV_C1X1", "0"),)),
    _case(1, 1, 128, 16, 132, 126, 1, 2, BF16, "f: d:addin w:", (None, 542, None)),
    _case(1, 1, 128, 32, 132, 126, 1, 2, BF16, "f: d:addin w:", (None, 642, None)),
    _case(1, 1, 128, 64, 132, 126, 1, 2, BF16, "f: d:addin+win w:", (None, 2007, None)),
    _case(1, 1, 128, 16, 132, 126, 3, 2, BF16, "f: d:add w:", (None, 4542, None)),
    _case(1, 1, 128, 32, 132, 126, 3, 2, BF16, "f: d:plain w:", (None, 4642, None)),
    _case(1, 1, 128, 64, 132, 126, 3, 2, BF16, "f: d:drelu+win w:", (None, 6007, None)),
    # ---- conv_res.hip: the resident-filter kernels (64 | 16 -> <= 64 channels, 3x3 stride 1)
    _case(2, 3, 16, 48, 12, 20, 3, 1, BF16, "f:stats+add d: w:", (1005, None, 7109), (("PMOE_CONV_C16", "0"),)),
    _case(2, 3, 64, 64, 12, 20, 3, 1, BF16, "f:stats+add+win d: w:", (1007, None, None), (("PMOE_RES_DMA", "0"),)),
    _case(1, 5, 64, 56, 24, 40, 3, 1, BF16, "f:bias d: w:", (1007, None, None), (("PMOE_RES_DMA", "0"),)),
    _case(2, 3, 64, 64, 12, 20, 3, 1, BF16, "f:stats+add d:dbn w:", (1107, 1107, None), (("PMOE_RES_PIPE", "0"),)),
    _case(1, 4, 64, 64, 40, 24, 3, 1, BF16, "f:bias d:dbn+bias+pimg w:", (1117, 1117, None), (("PMOE_RES_PIPE", "0"),)),
    _case(2, 3, 64, 64, 12, 20, 3, 1, BF16, "f:stats d:dbn+win w:", (1207, 1247, 7309)),
    _case(1, 2, 64, 56, 40, 72, 3, 1, BF16, "f:bias d: w:", (1217, None, None)),
    _case(1, 2, 64, 64, 40, 72, 3, 1, BF16, "f: d:addin w:", (None, 1227, None)),
    _case(1, 2, 64, 64, 40, 72, 3, 1, BF16, "f:add+win d:plain w:", (1227, 1207, None)),
    _case(1, 3, 64, 64, 24, 40, 3, 1, BF16, "f:inbn+stats d:dbn+bias+pimg w:", (1267, 1257, None)),
    _case(2, 5, 64, 64, 16, 16, 3, 1, BF16, "f:inbn+stats d: w:", (1267, None, 7309)),
    _case(1, 2, 16, 64, 40, 72, 3, 1, BF16, "f: d:bias w:", (None, 1217, None)),
    # ---- conv3x3_c16_kernel
    _case(2, 3, 16, 48, 12, 40, 3, 1, BF16, "f:stats+win d: w:", (1316, None, 7109)),
    _case(1, 5, 16, 64, 16, 33, 3, 1, BF16, "f:stats+shared d: w:", (1316, None, None)),
    _case(1, 1, 16, 16, 64, 66, 3, 1, BF16, "f: d:plain w:", (None, 1316, None)),
    _case(1, 1, 16, 16, 64, 66, 3, 1, BF16, "f: d:add w:", (None, 1005, None)),
    # ---- conv1x1_direct_kernel<MT[, INBN]>
    _case(2, 3, 64, 48, 40, 72, 1, 1, BF16, "f:stats+bias+win d: w:", (1402, None, 6106)),
    _case(1, 3, 128, 128, 56, 52, 1, 1, BF16, "f:stats d:plain w:", (1404, 1404, None)),
    _case(1, 4, 192, 64, 96, 90, 1, 2, BF16, "f:stats+shared d: w:", (1402, None, None)),
    _case(1, 3, 64, 16, 56, 52, 1, 1, BF16, "f:inbn+bias+win d: w:", (1412, None, None)),
    _case(2, 2, 128, 128, 64, 66, 1, 1, BF16, "f:inbn+stats d: w:", (1414, None, None)),
    _case(2, 4, 64, 32, 64, 32, 1, 1, BF16, "f:shuf+bias d: w:", (1452, None, None)),
    _case(1, 3, 128, 128, 64, 64, 1, 1, BF16, "f:shuf+inbn d: w:", (1464, None, None)),
    _case(1, 3, 128, 128, 64, 64, 1, 1, BF16, "f:shuf d: w:", (1454, None, None)),
    _case(1, 5, 64, 64, 32, 64, 1, 1, BF16, "f:shuf+inbn+bias d: w:", (1462, None, None)),
    # ---- conv_dma.hip: 256-pixel x 128-channel tiles over whole 64-channel chunks, >= 4096 pixels per expert.  A forward launch
    #      needs >= 128 output channels, a data gradient >= 128 input channels of the layer: one chunk each, but for the first case
    #      (two chunks on both: 1.3 GFLOP, the one case over the 0.5 GFLOP the others keep to)
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:stats d:plain w:", (5047, 5047, 7309)),
    _case(1, 3, 64, 128, 40, 36, 3, 1, BF16, "f:stats d: w:", (5057, None, None), MF16),
    _case(1, 17, 64, 128, 16, 16, 3, 1, BF16, "f:stats d: w:", (5007, None, 7309), DMA_ONE_TILE),
    _case(1, 3, 64, 120, 40, 36, 3, 1, BF16, "f:bias+relu+add+win d: w:", (5007, None, None)),
    _case(1, 3, 64, 128, 40, 36, 3, 1, BF16, "f:add+stats d: w:", (5007, None, None)),
    _case(1, 3, 128, 64, 40, 36, 3, 1, BF16, "f: d:drelu+win w:", (None, 5007, None)),
    _case(1, 17, 128, 64, 16, 16, 3, 1, BF16, "f: d:addin w:", (None, 5007, None)),
    _case(1, 3, 128, 64, 40, 36, 3, 1, BF16, "f: d:dbn w:", (None, 5007, None)),
    _case(1, 17, 64, 128, 16, 16, 3, 1, BF16, "f:add d: w:", (5017, None, None), MF16),
    _case(1, 17, 128, 64, 16, 16, 3, 1, BF16, "f: d:dbn+bias w:", (None, 5017, None), MF16),
    _case(1, 3, 128, 64, 40, 36, 3, 1, BF16, "f: d:dbn+win w:", (None, 5017, None), MF16),
    _case(1, 3, 64, 128, 40, 36, 3, 1, BF16, "f:stats d: w:", (5027, None, None), DMA_PRODUCER),
    _case(1, 17, 64, 128, 16, 16, 3, 1, BF16, "f:stats d: w:", (5037, None, None), MF16 + DMA_PRODUCER),
    _case(1, 3, 128, 64, 40, 36, 3, 1, BF16, "f: d:plain w:", (None, 5037, None), MF16 + DMA_PRODUCER),
    _case(2, 3, 128, 56, 40, 36, 3, 1, BF16, "f:stats d: w:", (5067, None, None)),
    _case(1, 17, 192, 64, 16, 16, 3, 1, BF16, "f:stats+win d: w:", (5067, None, None)),
    _case(1, 2, 16, 128, 64, 34, 3, 1, BF16, "f: d:plain w:", (None, 5067, None)),
    _case(1, 3, 64, 128, 81, 71, 3, 2, BF16, "f:stats d: w:", (5207, None, None)),
    _case(1, 1, 64, 128, 128, 130, 3, 2, BF16, "f:bias+relu+add d: w:", (5207, None, None)),
    _case(1, 1, 128, 64, 132, 126, 3, 2, BF16, "f: d:add w:", (None, 9207, None)),
    # ---- every form on every code that accepts it (tests/test_conv_cpu.py enumerates what the planner accepts per code and dtype);
    #      with statistics where the skinny GEMM would otherwise take the small shape
    _case(2, 2, 16, 128, 7, 9, 1, 2, BF16, "f:drelu+stats d: w:", (522, None, None)),
    _case(2, 2, 16, 128, 7, 9, 1, 2, BF16, "f:addin+stats+win d: w:", (522, None, None)),
    _case(2, 3, 16, 16, 7, 5, 1, 1, BF16, "f:drelu+stats d: w:", (541, None, None)),
    _case(2, 3, 16, 16, 7, 5, 1, 1, BF16, "f:addin+stats d: w:", (541, None, None)),
    _case(2, 1, 32, 128, 8, 8, 3, 1, BF16, "f:drelu+stats+win d: w:", (622, None, None)),
    _case(2, 1, 32, 128, 8, 8, 3, 1, BF16, "f:addin+stats d: w:", (622, None, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f:drelu+stats d: w:", (641, None, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f:addin+stats d: w:", (641, None, None)),
    _case(1, 2, 64, 128, 9, 9, 3, 2, BF16, "f:drelu+stats+win d: w:", (722, None, None)),
    _case(1, 2, 64, 128, 9, 9, 3, 2, BF16, "f:addin+stats d: w:", (722, None, None)),
    _case(2, 3, 64, 48, 9, 9, 1, 1, BF16, "f:shared+stats d: w:", (741, None, None)),
    _case(2, 3, 64, 64, 12, 20, 3, 1, BF16, "f:addin+stats+win d:dbn+win w:", (1107, 1107, None), (("PMOE_RES_PIPE", "0"),)),
    _case(1, 4, 64, 64, 40, 24, 3, 1, BF16, "f:bias+win d:dbn+bias+pimg+win w:", (1117, 1117, None), (("PMOE_RES_PIPE", "0"),)),
    _case(1, 2, 64, 56, 40, 72, 3, 1, BF16, "f:bias+win d: w:", (1217, None, None)),
    _case(1, 3, 64, 64, 24, 40, 3, 1, BF16, "f:inbn+stats+win d:dbn+bias+pimg+win w:", (1267, 1257, None)),
    _case(1, 2, 64, 64, 40, 72, 3, 1, BF16, "f:stats+win d: w:", (1207, None, None)),
    _case(1, 3, 128, 128, 56, 52, 1, 1, BF16, "f:stats+win d:bias+win w:", (1404, 1404, None)),
    _case(2, 2, 128, 128, 64, 66, 1, 1, BF16, "f:inbn+bias+win d: w:", (1414, None, None)),
    _case(1, 3, 128, 128, 64, 64, 1, 1, BF16, "f:shuf+bias+win d: w:", (1454, None, None)),
    _case(1, 3, 128, 128, 64, 64, 1, 1, BF16, "f:shuf+inbn+win d: w:", (1464, None, None)),
    _case(2, 4, 64, 32, 64, 32, 1, 1, BF16, "f:shuf+win d: w:", (1452, None, None)),
    _case(1, 5, 64, 64, 32, 64, 1, 1, BF16, "f:shuf+inbn+win d: w:", (1462, None, None)),
    _case(1, 3, 64, 128, 40, 36, 3, 1, BF16, "f:stats d: w:", (5017, None, None), MF16 + DMA_ONE_TILE),
    # ---- conv_dma.hip over SEVERAL 64-channel chunks (the patch-buffer alternation, the next chunk's prefetch, the residual
    #      prefetched under the last chunk): 128 input channels at the launch, 1.2 - 1.3 GFLOP each
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:add+win d:addin w:", (5007, 5007, None), DMA_ONE_TILE),
    _case(1, 17, 128, 128, 16, 16, 3, 1, BF16, "f:bias+relu+add d:drelu+win w:", (5017, 5017, None), MF16),
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:stats+win d:plain+win w:", (5027, 5027, None), DMA_PRODUCER),
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:stats+win d:plain w:", (5037, 5037, None), MF16 + DMA_PRODUCER),
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:stats+win d:plain+win w:", (5057, 5057, None), MF16),
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:stats+win d: w:", (5047, None, None)),
    _case(1, 1, 128, 128, 128, 130, 3, 2, BF16, "f:add+stats+win d:plain+win w:", (5207, 9207, None)),
    _case(1, 1, 128, 128, 132, 126, 3, 2, BF16, "f:bias+win d:addin w:", (5207, 9207, None)),
    # ---- a weight-gradient workgroup that walks several pixel blocks before its K-split slab is folded (264 blocks on 132 slices)
    _case(1, 3, 64, 64, 88, 256, 1, 1, BF16, "f: d: w:", (None, None, 6106)),
    _case(1, 1, 16, 16, 64, 66, 3, 1, BF16, "f: d:addin+win w:", (None, 1005, None)),
    _case(2, 3, 16, 48, 12, 20, 3, 1, BF16, "f:shared+stats d: w:", (1005, None, None), (('PMOE_CONV_C16', '0'),)),
    _case(1, 5, 64, 56, 24, 40, 3, 1, BF16, "f:addin d: w:", (1007, None, None), (('PMOE_RES_DMA', '0'),)),
    _case(2, 3, 64, 64, 12, 20, 3, 1, BF16, "f:shared+stats d: w:", (1007, None, None), (('PMOE_RES_DMA', '0'),)),
    _case(1, 3, 128, 128, 56, 52, 1, 1, BF16, "f:bias+stats d: w:", (1404, None, None)),
    _case(1, 3, 128, 128, 56, 52, 1, 1, BF16, "f:shared+stats d: w:", (1404, None, None)),
    _case(1, 1, 64, 128, 64, 66, 1, 1, BF16, "f:bias+stats d: w:", (2007, None, None), (('PMOE_CONV_C1X1', '0'),)),
    _case(1, 1, 64, 128, 64, 66, 1, 1, BF16, "f:drelu d: w:", (2007, None, None), (('PMOE_CONV_C1X1', '0'),)),
    _case(1, 1, 64, 128, 64, 66, 1, 1, BF16, "f:bias+relu+stats d: w:", (2007, None, None), (('PMOE_CONV_C1X1', '0'),)),
    _case(1, 1, 64, 128, 64, 66, 1, 1, BF16, "f:shared+stats d: w:", (2007, None, None), (('PMOE_CONV_C1X1', '0'),)),
    _case(1, 2, 128, 16, 13, 9, 3, 2, BF16, "f: d:add+win w:", (None, 4522, None)),
    _case(1, 2, 128, 16, 13, 9, 3, 2, BF16, "f: d:bias w:", (None, 4522, None)),
    _case(1, 2, 128, 16, 13, 9, 3, 2, BF16, "f: d:drelu w:", (None, 4522, None)),
    _case(1, 2, 64, 48, 13, 9, 3, 2, BF16, "f: d:add w:", (None, 4541, None)),
    _case(1, 2, 64, 48, 13, 9, 3, 2, BF16, "f: d:bias+win w:", (None, 4541, None)),
    _case(1, 2, 64, 48, 13, 9, 3, 2, BF16, "f: d:drelu w:", (None, 4541, None)),
    _case(1, 1, 128, 16, 132, 126, 3, 2, BF16, "f: d:addin w:", (None, 4542, None)),
    _case(1, 1, 128, 16, 132, 126, 3, 2, BF16, "f: d:bias w:", (None, 4542, None)),
    _case(1, 1, 128, 16, 132, 126, 3, 2, BF16, "f: d:drelu+win w:", (None, 4542, None)),
    _case(1, 2, 128, 32, 13, 9, 3, 2, BF16, "f: d:addin w:", (None, 4622, None)),
    _case(1, 2, 128, 32, 13, 9, 3, 2, BF16, "f: d:bias+win w:", (None, 4622, None)),
    _case(1, 2, 128, 32, 13, 9, 3, 2, BF16, "f: d:drelu w:", (None, 4622, None)),
    _case(1, 2, 128, 16, 9, 7, 3, 2, F32, "f: d:add w:", (None, 4622, None)),
    _case(1, 2, 128, 16, 9, 7, 3, 2, F32, "f: d:addin w:", (None, 4622, None)),
    _case(1, 2, 128, 16, 9, 7, 3, 2, F32, "f: d:bias+win w:", (None, 4622, None)),
    _case(1, 2, 128, 16, 9, 7, 3, 2, F32, "f: d:drelu w:", (None, 4622, None)),
    _case(1, 2, 64, 32, 13, 9, 3, 2, BF16, "f: d:add w:", (None, 4641, None)),
    _case(1, 2, 64, 32, 13, 9, 3, 2, BF16, "f: d:addin w:", (None, 4641, None)),
    _case(1, 2, 64, 32, 13, 9, 3, 2, BF16, "f: d:bias w:", (None, 4641, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f: d:addin w:", (None, 4641, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f: d:bias w:", (None, 4641, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f: d:drelu w:", (None, 4641, None)),
    _case(1, 1, 128, 32, 132, 126, 3, 2, BF16, "f: d:add+win w:", (None, 4642, None)),
    _case(1, 1, 128, 32, 132, 126, 3, 2, BF16, "f: d:addin w:", (None, 4642, None)),
    _case(1, 1, 128, 32, 132, 126, 3, 2, BF16, "f: d:bias w:", (None, 4642, None)),
    _case(1, 1, 128, 32, 132, 126, 3, 2, BF16, "f: d:drelu w:", (None, 4642, None)),
    _case(1, 2, 128, 64, 7, 7, 3, 2, BF16, "f: d:add w:", (None, 4722, None)),
    _case(1, 2, 128, 64, 7, 7, 3, 2, BF16, "f: d:addin w:", (None, 4722, None)),
    _case(1, 2, 128, 64, 7, 7, 3, 2, BF16, "f: d:bias+win w:", (None, 4722, None)),
    _case(1, 2, 128, 32, 7, 7, 3, 2, F32, "f: d:addin w:", (None, 4722, None)),
    _case(1, 2, 128, 32, 7, 7, 3, 2, F32, "f: d:bias+win w:", (None, 4722, None)),
    _case(1, 2, 128, 32, 7, 7, 3, 2, F32, "f: d:drelu w:", (None, 4722, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f: d:addin w:", (None, 4741, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f: d:bias w:", (None, 4741, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f: d:drelu w:", (None, 4741, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f: d:add w:", (None, 4741, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f: d:addin w:", (None, 4741, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f: d:drelu w:", (None, 4741, None)),
    _case(1, 17, 64, 128, 16, 16, 3, 1, BF16, "f:addin d: w:", (5017, None, None), MF16),
    _case(1, 17, 64, 128, 16, 16, 3, 1, BF16, "f:drelu d: w:", (5017, None, None), MF16),
    _case(1, 17, 64, 128, 16, 16, 3, 1, BF16, "f:bias+relu d: w:", (5017, None, None), MF16),
    _case(1, 3, 64, 128, 81, 71, 3, 2, BF16, "f:drelu d: w:", (5207, None, None)),
    _case(2, 2, 16, 128, 7, 9, 1, 2, BF16, "f:add+stats d: w:", (522, None, None)),
    _case(2, 2, 16, 128, 7, 9, 1, 2, BF16, "f:bias+stats d: w:", (522, None, None)),
    _case(2, 3, 16, 16, 7, 5, 1, 1, BF16, "f:add+stats d: w:", (541, None, None)),
    _case(2, 3, 16, 16, 7, 5, 1, 1, BF16, "f:bias+stats d: w:", (541, None, None)),
    _case(2, 3, 16, 16, 7, 5, 1, 1, BF16, "f:bias+relu+stats d: w:", (541, None, None)),
    _case(2, 3, 16, 16, 7, 5, 1, 1, BF16, "f:shared+stats d: w:", (541, None, None)),
    _case(1, 1, 16, 128, 64, 66, 1, 1, BF16, "f:bias+stats d: w:", (542, None, None)),
    _case(1, 1, 16, 128, 64, 66, 1, 1, BF16, "f:drelu d: w:", (542, None, None)),
    _case(1, 1, 16, 128, 64, 66, 1, 1, BF16, "f:bias+relu+stats d: w:", (542, None, None)),
    _case(1, 1, 16, 128, 64, 66, 1, 1, BF16, "f:shared+stats d: w:", (542, None, None)),
    _case(2, 1, 32, 128, 8, 8, 3, 1, BF16, "f:bias+stats d: w:", (622, None, None)),
    _case(1, 2, 16, 128, 9, 7, 1, 2, F32, "f:add d: w:", (622, None, None)),
    _case(1, 2, 16, 128, 9, 7, 1, 2, F32, "f:addin d: w:", (622, None, None)),
    _case(1, 2, 16, 128, 9, 7, 1, 2, F32, "f:drelu d: w:", (622, None, None)),
    _case(1, 2, 16, 128, 9, 7, 1, 2, F32, "f:shared d: w:", (622, None, None)),
    _case(1, 2, 16, 128, 9, 7, 1, 2, F32, "f:stats d: w:", (622, None, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f:add+stats d: w:", (641, None, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f:shared+stats d: w:", (641, None, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f:add+stats d: w:", (641, None, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f:addin d: w:", (641, None, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f:drelu d: w:", (641, None, None)),
    _case(2, 3, 16, 16, 7, 5, 3, 2, F32, "f:bias+relu+stats d: w:", (641, None, None)),
    _case(1, 1, 32, 128, 64, 66, 1, 1, BF16, "f:add+win d: w:", (642, None, None)),
    _case(1, 1, 32, 128, 64, 66, 1, 1, BF16, "f:drelu d: w:", (642, None, None)),
    _case(1, 1, 32, 128, 64, 66, 1, 1, BF16, "f:shared d: w:", (642, None, None)),
    _case(1, 1, 32, 128, 64, 66, 1, 1, BF16, "f:stats d: w:", (642, None, None)),
    _case(1, 2, 64, 128, 9, 9, 3, 2, BF16, "f:add+stats d: w:", (722, None, None)),
    _case(1, 2, 64, 128, 9, 9, 3, 2, BF16, "f:bias+stats d: w:", (722, None, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f:add+stats d: w:", (722, None, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f:addin d: w:", (722, None, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f:bias+stats d: w:", (722, None, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f:drelu d: w:", (722, None, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f:bias+relu+stats d: w:", (722, None, None)),
    _case(1, 3, 32, 128, 7, 7, 3, 2, F32, "f:shared+stats d: w:", (722, None, None)),
    _case(2, 2, 16, 128, 7, 9, 1, 2, BF16, "f: d:add w:", (None, 741, None)),
    _case(1, 2, 16, 128, 9, 7, 1, 2, F32, "f: d:bias w:", (None, 741, None)),
    _case(2, 2, 32, 32, 8, 8, 3, 1, F32, "f:bias+relu+stats d: w:", (741, None, None)),
    _case(2, 2, 32, 32, 8, 8, 3, 1, F32, "f:shared+stats d: w:", (741, None, None)),
    _case(1, 1, 128, 64, 132, 126, 3, 2, BF16, "f: d:addin w:", (None, 9207, None)),
    _case(1, 1, 128, 64, 132, 126, 3, 2, BF16, "f: d:bias w:", (None, 9207, None)),
    # ---- conv_wgrad.hip: what the cases above do not reach
    _case(1, 2, 64, 64, 32, 8, 3, 1, BF16, "f: d: w:", (None, None, 7009)),
    _case(2, 3, 16, 48, 20, 36, 3, 1, BF16, "f: d: w:pimg", (None, None, 7109)),
    _case(2, 3, 16, 48, 20, 36, 3, 1, BF16, "f: d: w:pimg+bn", (None, None, 7209)),
    _case(1, 2, 8, 64, 16, 16, 3, 1, BF16, "f: d: w:pimg+bn", (None, None, 7209)),
    _case(2, 2, 64, 128, 20, 36, 3, 1, BF16, "f: d: w:pimg+win", (None, None, 7309)),
    _case(1, 2, 64, 64, 16, 16, 3, 1, F32, "f: d: w:", (None, None, 6912)),
    # ---- gemm_skinny_kernel<4> (csrc/gemm_skinny.hip): bf16 launches without statistics of <= 3200 output rows per expert.  One
    #      workgroup per 64 rows x 64 channels of one expert; wave w takes the 16-channel k-slices w, w + 4, ... of every tap.
    #      The MLP form (1x1 images): one k-slice (waves 1-3 add zero tiles) and one valid channel vector of 64; a ragged second
    #      row block, an idle fourth wave and a second column block with 8 valid channels; three row blocks with a fifth slice for
    #      wave 0 (past the `#pragma unroll 4`); a shared input
    _case(2, 5, 16, 8, 1, 1, 1, 1, BF16, "f:bias d: w:", (3000, None, None)),
    _case(3, 70, 48, 72, 1, 1, 1, 1, BF16, "f:bias+relu+win d: w:", (3000, None, None)),
    _case(1, 130, 272, 64, 1, 1, 1, 1, BF16, "f:add d:addin w:", (3000, 3000, None)),
    _case(2, 7, 80, 24, 1, 1, 1, 1, BF16, "f:shared+bias d: w:", (3000, None, None)),
    #      the tap loop: borders on all sides; odd sides at stride 2; 1x1 at stride 2; 75 and 196 rows, so that a 64-row block
    #      spans image boundaries and ends ragged
    _case(2, 1, 16, 16, 7, 5, 3, 1, BF16, "f:bias+relu d:add+win w:", (3000, 3000, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f:add+win d: w:", (3000, None, None)),
    _case(2, 2, 48, 32, 10, 6, 1, 2, BF16, "f:addin d: w:", (3000, None, None)),
    _case(1, 3, 16, 16, 5, 5, 3, 1, BF16, "f:drelu+win d:drelu w:", (3000, 3000, None)),
    _case(1, 1, 16, 16, 14, 14, 3, 1, BF16, "f:shared d:bias w:", (3000, 3000, None)),
    #      exactly 3200 rows per expert, the most the kernel takes (2 x 40 x 41: tests/test_conv_cpu.py, plan only)
    _case(1, 2, 16, 16, 40, 40, 1, 1, BF16, "f:bias d: w:", (3000, None, None)),
    #      the MLP epilogue forms (conv_ref.mlp_epilogue), on the dyadic kind: bias + elu + drop is the MLP layer, delu + drop its
    #      data gradient (a data gradient reduces over the layer's outputs: whole k-slices of 16, so not on every shape)
    _case(2, 5, 16, 8, 1, 1, 1, 1, BF16, "f:elu+bias+drop d: w:", (3000, None, None)),
    _case(3, 70, 48, 72, 1, 1, 1, 1, BF16, "f:bias+tanh+dropL+win d: w:", (3000, None, None)),
    _case(1, 130, 272, 64, 1, 1, 1, 1, BF16, "f:sigmoid d:dsigmoid+dropL w:", (3000, 3000, None)),
    _case(1, 130, 272, 64, 1, 1, 1, 1, BF16, "f:elu+dropL d:delu+win w:", (3000, 3000, None)),
    _case(2, 7, 80, 24, 1, 1, 1, 1, BF16, "f:shared+elu d: w:", (3000, None, None)),
    _case(2, 1, 16, 16, 7, 5, 3, 1, BF16, "f:bias+sigmoid+dropE d:delu+drop w:", (3000, 3000, None)),
    _case(2, 1, 16, 16, 7, 5, 3, 1, BF16, "f:tanh+drop d:dtanh w:", (3000, 3000, None)),
    _case(1, 3, 16, 16, 5, 5, 3, 1, BF16, "f:drop+win d:dtanh+drop w:", (3000, 3000, None)),
    _case(1, 1, 16, 16, 14, 14, 3, 1, BF16, "f:bias+relu+dropL d:drelu+drop+win w:", (3000, 3000, None)),
    _case(1, 1, 16, 16, 14, 14, 3, 1, BF16, "f:sigmoid+win d:dsigmoid w:", (3000, 3000, None)),
    _case(1, 3, 32, 64, 9, 7, 3, 2, BF16, "f:tanh d: w:", (3000, None, None)),
    # ---- the other two copies of that epilogue (EPILOGUE_COPY): conv_igemm.hip -- a 1x1 launch just over 3200 rows in bf16, the
    #      f32 MLP path -- and conv_dma_epilogue.inc (two-phase f32 read-out)
    _case(1, 51, 16, 16, 8, 8, 1, 1, BF16, "f:bias+elu+drop d:delu+drop w:", (541, 541, None)),
    _case(1, 51, 16, 16, 8, 8, 1, 1, BF16, "f:tanh+dropL+win d:dtanh+win w:", (541, 541, None)),
    _case(1, 51, 16, 16, 8, 8, 1, 1, BF16, "f:sigmoid d:dsigmoid+dropL w:", (541, 541, None)),
    _case(2, 5, 16, 8, 1, 1, 1, 1, F32, "f:elu+bias+dropE d: w:", (641, None, None)),
    _case(3, 70, 48, 72, 1, 1, 1, 1, F32, "f:bias+tanh+win d: w:", (622, None, None)),
    _case(1, 130, 272, 64, 1, 1, 1, 1, F32, "f:sigmoid+dropL d:dsigmoid w:", (641, 741, None)),
    _case(1, 130, 272, 64, 1, 1, 1, 1, F32, "f: d:delu+drop w:", (None, 741, None)),
    _case(1, 130, 272, 64, 1, 1, 1, 1, F32, "f: d:dtanh+drop+win w:", (None, 741, None)),
    _case(1, 3, 64, 128, 40, 36, 3, 1, BF16, "f:bias+elu+drop d: w:", (5007, None, None)),
    _case(1, 3, 64, 128, 40, 36, 3, 1, BF16, "f:tanh+dropL+win d: w:", (5007, None, None)),
    _case(1, 3, 64, 128, 40, 36, 3, 1, BF16, "f:sigmoid d: w:", (5007, None, None)),
    _case(1, 3, 128, 64, 40, 36, 3, 1, BF16, "f: d:delu+drop w:", (None, 5007, None)),
    _case(1, 3, 128, 64, 40, 36, 3, 1, BF16, "f: d:dtanh+win w:", (None, 5007, None)),
    _case(1, 3, 128, 64, 40, 36, 3, 1, BF16, "f: d:dsigmoid+dropL w:", (None, 5007, None)),
    # ---- conv_igemm_kernel<T, 7, 4, 2> (742): >= 4096 pixels per expert on maps so small that the halo patch of a 256-pixel tile
    #      (16 images of 6 x 6 pixels) no longer fits twice on a CU, so the LITE tile declines -- a 4 x 4 last stage at 256 images
    #      per expert; one and two channel chunks (the second: chunk prefetch), and as a parity class of a stride-2 data gradient
    _case(1, 256, 64, 128, 4, 4, 3, 1, BF16, "f:stats+win d: w:", (742, None, None)),
    _case(1, 256, 64, 128, 4, 4, 3, 1, BF16, "f:bias+relu+add d: w:", (742, None, None)),
    _case(2, 256, 64, 128, 4, 4, 3, 1, BF16, "f:shared+stats d: w:", (742, None, None)),
    _case(1, 256, 128, 128, 4, 4, 3, 1, BF16, "f:drelu+stats d: w:", (742, None, None)),
    _case(1, 256, 128, 64, 4, 4, 3, 1, BF16, "f: d:addin+win w:", (None, 742, None)),
    _case(1, 256, 128, 64, 8, 8, 3, 2, BF16, "f: d:add+win w:", (None, 4742, None)),
    _case(1, 256, 128, 64, 8, 8, 3, 2, BF16, "f: d:addin w:", (None, 4742, None)),
    _case(1, 256, 128, 64, 8, 8, 3, 2, BF16, "f: d:bias w:", (None, 4742, None)),
    _case(1, 256, 128, 64, 8, 8, 3, 2, BF16, "f: d:drelu w:", (None, 4742, None)),
    # ---- float32 522 and 541 as PLAIN launches (8-channel reductions; the rows above reach them as parity classes only)
    _case(2, 2, 8, 128, 7, 7, 3, 1, F32, "f:stats+win d: w:", (522, None, None)),
    _case(2, 2, 8, 128, 7, 7, 3, 1, F32, "f:bias+relu+add d: w:", (522, None, None)),
    _case(2, 2, 8, 128, 7, 7, 3, 1, F32, "f:drelu+shared+stats d: w:", (522, None, None)),
    _case(2, 2, 8, 16, 7, 7, 3, 1, F32, "f:stats+win d: w:", (541, None, None)),
    _case(2, 2, 8, 16, 7, 7, 3, 1, F32, "f:bias+relu+add d: w:", (541, None, None)),
    _case(2, 2, 8, 16, 7, 7, 3, 1, F32, "f:drelu+shared+stats d: w:", (541, None, None)),
    #      ... and as data gradients of layers with 8 outputs, accumulated in place; the float32 forms of their parity classes
    _case(2, 2, 128, 8, 7, 7, 3, 1, F32, "f: d:addin w:", (None, 522, None)),
    _case(2, 2, 16, 8, 7, 7, 3, 1, F32, "f: d:addin+win w:", (None, 541, None)),
    _case(1, 2, 128, 8, 9, 7, 3, 2, F32, "f: d:add w:", (None, 4522, None)),
    _case(1, 2, 128, 8, 9, 7, 3, 2, F32, "f: d:bias w:", (None, 4522, None)),
    _case(1, 2, 128, 8, 9, 7, 3, 2, F32, "f: d:drelu w:", (None, 4522, None)),
    _case(1, 2, 16, 8, 9, 7, 3, 2, F32, "f: d:addin w:", (None, 4541, None)),
    _case(1, 2, 16, 8, 9, 7, 3, 2, F32, "f: d:bias w:", (None, 4541, None)),
    _case(1, 2, 16, 8, 9, 7, 3, 2, F32, "f: d:drelu w:", (None, 4541, None)),
    # ---- e4m3 weights, bfloat16 input converted by the patch loader (conv_igemm_body<bf16, ..., fp8>): 8000 + the tile code, in
    #      64- and 128-channel chunks.  Per code: statistics on channel windows; bias + ReLU + side input; the ReLU' mask on a
    #      shared input.  Each also on the select kind: every converting loader, chunk width and tap meets every e4m3 value, tie
    #      and overflow.  One case under in_scale 32.
    _case(2, 3, 64, 48, 9, 7, 3, 2, BF16, "f:f8+stats+win d: w:", (8641, None, None)),
    _case(2, 3, 64, 48, 9, 7, 3, 2, BF16, "f:f8+bias+relu+add d: w:", (8641, None, None)),
    _case(2, 3, 64, 48, 9, 7, 3, 2, BF16, "f:f8+drelu+shared+stats d: w:", (8641, None, None)),
    _case(1, 3, 128, 64, 7, 7, 3, 1, BF16, "f:f8+sc32+stats+win d: w:", (8741, None, None)),
    _case(1, 3, 128, 64, 7, 7, 3, 1, BF16, "f:f8+bias+relu+add d: w:", (8741, None, None)),
    _case(2, 3, 128, 64, 7, 7, 3, 1, BF16, "f:f8+drelu+shared+stats d: w:", (8741, None, None)),
    _case(2, 1, 64, 128, 8, 8, 3, 1, BF16, "f:f8+stats+win d: w:", (8622, None, None)),
    _case(2, 1, 64, 128, 8, 8, 3, 1, BF16, "f:f8+bias+relu+add d: w:", (8622, None, None)),
    _case(2, 1, 64, 128, 8, 8, 3, 1, BF16, "f:f8+drelu+shared+stats d: w:", (8622, None, None)),
    _case(1, 2, 128, 128, 9, 9, 3, 2, BF16, "f:f8+stats+win d: w:", (8722, None, None)),
    _case(1, 2, 128, 128, 9, 9, 3, 2, BF16, "f:f8+bias+relu+add d: w:", (8722, None, None)),
    _case(2, 2, 128, 128, 9, 9, 3, 2, BF16, "f:f8+drelu+shared+stats d: w:", (8722, None, None)),
    _case(1, 1, 64, 128, 64, 66, 1, 1, BF16, "f:f8+stats+win d: w:", (8642, None, None)),
    _case(1, 1, 64, 128, 128, 130, 3, 2, BF16, "f:f8+bias+relu+add d: w:", (8642, None, None)),
    _case(2, 1, 64, 128, 64, 66, 1, 1, BF16, "f:f8+drelu+shared+stats d: w:", (8642, None, None)),
    _case(1, 1, 128, 128, 64, 66, 1, 1, BF16, "f:f8+stats+win d: w:", (10007, None, None)),
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:f8+bias+relu+add d: w:", (10007, None, None)),
    _case(2, 1, 128, 128, 64, 66, 1, 1, BF16, "f:f8+drelu+shared+stats d: w:", (10007, None, None)),
    _case(1, 256, 128, 128, 4, 4, 3, 1, BF16, "f:f8+stats+win d: w:", (8742, None, None)),
    _case(1, 256, 128, 128, 4, 4, 3, 1, BF16, "f:f8+bias+relu+add d: w:", (8742, None, None)),
    _case(2, 256, 128, 72, 4, 4, 3, 1, BF16, "f:f8+drelu+shared+stats d: w:", (8742, None, None)),
    #      ... accumulated in place (res == out)
    _case(2, 3, 64, 48, 9, 7, 3, 2, BF16, "f:f8+addin d: w:", (8641, None, None)),
    _case(1, 3, 128, 64, 7, 7, 3, 1, BF16, "f:f8+addin+win d: w:", (8741, None, None)),
    _case(2, 1, 64, 128, 8, 8, 3, 1, BF16, "f:f8+addin d: w:", (8622, None, None)),
    _case(1, 2, 128, 128, 9, 9, 3, 2, BF16, "f:f8+addin+stats d: w:", (8722, None, None)),
    _case(1, 1, 64, 128, 64, 66, 1, 1, BF16, "f:f8+addin d: w:", (8642, None, None)),
    _case(1, 1, 128, 128, 64, 66, 1, 1, BF16, "f:f8+addin d: w:", (10007, None, None)),
    _case(1, 256, 128, 72, 4, 4, 3, 1, BF16, "f:f8+addin+win d: w:", (8742, None, None)),
    # ---- e4m3 weights AND e4m3 input bytes on the block-scaled MFMA (conv3x3_dma_f8_kernel, 8507; it takes no side input): one and
    #      two 128-channel chunks, image groups of 16 x 16 maps, a ragged last channel vector block (120), channel windows on both
    #      sides (in_ld > cin: the 0x7f bytes beside the window are NaN).  On the select kind: all 254 non-NaN byte codes, which
    #      proves the byte decoding and the lane-half split of the instruction's operands
    _case(1, 3, 128, 128, 40, 36, 3, 1, BF16, "f:a8+stats d: w:", (8507, None, None)),
    _case(1, 17, 128, 128, 16, 16, 3, 1, BF16, "f:a8+bias+relu+stats+win d: w:", (8507, None, None)),
    _case(1, 3, 256, 128, 40, 36, 3, 1, BF16, "f:a8 d: w:", (8507, None, None)),
    _case(1, 3, 128, 120, 40, 36, 3, 1, BF16, "f:a8+bias+win d: w:", (8507, None, None)),
]
TILE_CODES = (522, 541, 542, 622, 641, 642, 722, 741, 742, 2007)
TILE_CODES_F8 = tuple(8000 + c for c in (622, 641, 642, 722, 741, 742, 2007))      # (e4m3 operands: 64- and 128-channel chunks only)


# The three copies of the MLP epilogue (mlp_epilogue), by plan code.  A code that is not here belongs to a kernel whose planner
# refuses every MLP form (conv_res.hip, conv_c16.hip, conv_c1x1.hip, and the producer-wave / persistent instantiations of
# conv_dma.hip, which take plain launches only): test_every_plan_code_of_the_grid_has_a_case asserts from the grid that no such
# code ever answers a descriptor with one of the forms, and that every (copy, dtype, form) the grid reaches has a case.  The
# LDS-DMA kernels do take them -- a 3x3 layer of >= 4096 pixels per expert with an activation or dropout runs on
# conv_dma_epilogue.inc's two-phase read-out (5007 | 5017 | 5207; the parity-class launches 9207 take the forward forms only).
# The kernels with e4m3 operands run the same two copies (8000 + a tile code: conv_igemm_body; 8507: conv_dma_epilogue.inc under
# DMA_OSCALE) and their planners accept the forms, but no case runs an MLP form on e4m3 operands: the dyadic inputs are not
# e4m3-exact, and the code is the copy the bfloat16 cases run.
EPILOGUE_COPY = {
    3000: "gemm_skinny.hip",
    **{c: "conv_igemm.hip" for c in TILE_CODES}, **{4000 + c: "conv_igemm.hip" for c in TILE_CODES},
    **{c: "conv_igemm.hip" for c in TILE_CODES_F8},
    **{c: "conv_dma_epilogue.inc" for c in (5007, 5017, 5207, 9207, 8507)},
}


def kinds_of(case):
    """the kinds a case runs on: the MLP forms on the dyadic kind, everything else on the lattice and unit kinds -- and a case
    with e4m3 operands on the select kind too"""
    fl = flags(case)
    if any(fl[k] and fl[k] & MLP_FLAGS for k in "fd"):
        return (DYADIC,)
    return KINDS + (SELECT,) if fl["f"] and fl["f"] & F8_FLAGS else KINDS


def case_id(case):
    sw = "".join(f"-{k[5:]}={v}" for k, v in case.switches)
    return (f"{case.E}x{case.ipe}-{case.cin}to{case.cout}-{case.H}x{case.W}-k{case.ks}s{case.stride}-"
            f"{'bf16' if case.dtype == BF16 else 'f32'}-{case.request.replace(' ', '_').replace(':', '.')}{sw}")


def flags(case):
    """{"f": set | None, "d": ..., "w": ...}: the flags of each launch; None = the launch is not run"""
    out = {}
    for part in case.request.split():
        k, v = part.split(":")
        out[k] = set(filter(None, v.split("+")))
    for i, k in enumerate("fdw"):
        if case.codes[i] is None:
            out[k] = None
        else:
            assert out.get(k) is not None, (case, k)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# generators

def value_range(kind, K):
    """largest absolute value of activations, weights and gradients of a reduction over K terms.  lattice: +-7 from K = 128 to
    1152 and +-3 above keep sum |x||w| below 2^24 and the outputs a few hundred large, where bfloat16 rounds integers both
    inexactly and on exact ties; shorter reductions need wider values for that"""
    if kind == "unit":
        return 1
    return 15 if K < 24 else 13 if K < 48 else 11 if K < 128 else 7 if K <= 1152 else 3


def _ints(g, shape, lim, kind):
    t = torch.randint(-lim, lim + 1, shape, generator=g).to(F64)
    if kind == "unit":
        t = t * (torch.randint(0, 8, shape, generator=g) < 3)            # +-1 | 0 | 0 (x 3/8 kept): a quarter non-zero
    return t + 0.0                                                       # (no negative zeros: -1 * False is one)


def bn_coefficients(g, Ebn, C, kind):
    """[4, Ebn, C] = mean, invstd, gamma * invstd, beta.  lattice: bn_ref.lattice_case's sets (mean: multiples of 1/4, beta:
    of 1/2, gamma * invstd in {-1, 1/2, 1, 2}, invstd in {1, 2}); unit: integers (the activation stays an integer)"""
    pick = lambda vals: torch.tensor(vals, dtype=F64)[torch.randint(0, len(vals), (Ebn, C), generator=g)]
    q = lambda lim, den: torch.randint(-lim, lim + 1, (Ebn, C), generator=g).to(F64) / den
    if kind == "unit":
        return torch.stack([q(1, 1), pick([1.0, 2.0]), pick([-1.0, 1.0]), q(1, 1)])
    return torch.stack([q(2, 4), pick([1.0, 2.0]), pick([-1.0, 0.5, 1.0, 2.0]), q(1, 2)])


def planted_z(g, shape, coef, bn_ipe, kind):
    """z [N, H, W, C] whose pre-activation (z - mean) * scale + beta sits exactly on the ReLU edge, one step of z above and one
    below for three of every eight elements (bn_ref.planted's pattern); the rest random on the lattice of the kind"""
    n, h, w, c = shape
    step = 1.0 if kind == "unit" else 0.25
    z = torch.randint(-8, 9, shape, generator=g).to(F64) / 4 if kind == "lattice" else _ints(g, shape, 1, "lattice")
    mean, _, scale, shift = (_per_image(k, bn_ipe) for k in coef)
    code = (torch.arange(n * h * w).reshape(n, h, w, 1) + torch.arange(c)) % 8 + 1
    code = torch.where((code != 4) & (code != 8), code, torch.zeros_like(code))
    off = torch.where((code & 3) == 2, step, torch.where((code & 3) == 3, -step, 0.0)).to(F64)
    z0 = mean - shift / scale + off
    on_lattice = (z0 / step == torch.round(z0 / step)) & (z0.abs() <= 4)       # (unit: beta / scale is an integer; always true)
    return torch.where((code >= 1) & (code <= 3) & on_lattice, z0, z)


def _window(t, win, extra=32, coff=16):
    """[..., C] -> ([..., C + extra] with NaN outside the window, coff) (win), or (t, 0)"""
    if not win:
        return t, 0
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + extra,), float("nan"), dtype=F64)
    buf[..., coff:coff + t.shape[-1]] = t
    return buf, coff


SENTINEL = -77.0


def _out_buffer(shape_c, cout, win, fill=None):
    """output buffer before the launch: rows of r16(cout) channels (+ 32 with win), SENTINEL everywhere (or ``fill``: the values
    an in-place accumulation finds, in the window); -> (buffer, out_coff)"""
    ld, coff = r16(cout) + (32 if win else 0), (16 if win else 0)
    buf = torch.full(shape_c + (ld,), SENTINEL, dtype=F64)
    if fill is not None:
        buf[..., coff:coff + cout] = fill
    return buf, coff


def _sparse_ints(g, shape, K):
    """integers of +-1 and +-2, non-zero with probability 4.8 / K: against weights uniform on the multiples of 1/64 in [-1, 1] a
    sum over K terms has a standard deviation of about 2 -- pre-activations all over (-8, 8), on some thousand distinct
    multiples of 1/64"""
    t = torch.randint(1, 3, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
    return (t * (torch.rand(shape, generator=g) < min(1.0, 4.8 / K))).to(F64) + 0.0


def _dyadic(g, shape):
    """multiples of 1/64 in [-1, 1]: exact in bfloat16"""
    return torch.randint(-64, 65, shape, generator=g).to(F64) / 64


def saved_output(g, shape, mode, drop_p, seed, dtype):
    """what a D-mode launch reads: the reference's own forward output of the matching activation (ReLU for PMOE_RES_DRELU) under
    the same drop_p, in storage precision, of pre-activations on the multiples of 1/64 -- with exact zeros among them, kept and
    dropped.  Standard deviation 1.5, narrower than the forward cases': 1 - u^2 and u (1 - u) of a SATURATED saved output cancel
    to a few bfloat16 steps of u, the carried error of u is then a visible share of the result, and the stored value of every
    such element is open between two neighbours -- few of them keep the launch under the cap on open elements"""
    z = (torch.randn(shape, generator=g, dtype=F64) * 96).round().clamp(-511, 511) / 64
    z.view(-1)[::37] = 0
    ep = mlp_epilogue(z, None, res_mode=RES_NONE, act=ACT_OF_DMODE[mode], drop_p=drop_p, seed=seed)
    return round_to(ep["value"], dtype), z


def _dyadic_launches(case):
    """launches() of a case that names an MLP form.  Forward: sparse integer activations, dyadic weights and biases; filter row 0
    of expert 0 and its bias are zero, so that exact zeros are among the pre-activations.  Data gradient: the same for dy and
    the filter, the residual is saved_output."""
    E, ipe, cin, cout, H, W, ks, stride, dtype = case[:9]
    fl = flags(case)
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id(case) + DYADIC)))
    N, pad = E * ipe, ks // 2
    Ho, Wo = out_size(H, ks, stride, pad), out_size(W, ks, stride, pad)
    out = {}

    def dropout(f, kw):
        for name in DROP_FLAGS:
            if name in f:
                kw.update(drop_p=DROP_P, seed=SEED_OF[name])

    f = fl["f"]
    if f is not None:
        assert not f - MLP_FLAGS - {"bias", "relu", "shared", "win"}, f
        shared, win = "shared" in f, "win" in f
        w = _dyadic(g, (E, cout, cin, ks, ks))
        w[0, 0] = 0
        L = {"w": w, "bias": None, "res": None, "bn_coef": None, "res_is_out": False}
        kw = dict(cin=cin, cout=cout, ipe=ipe, ks=ks, stride=stride, pad=pad, dtype=dtype, in_shared=shared, stats=False)
        if "bias" in f:
            L["bias"] = _dyadic(g, (E, cout))
            L["bias"][0, 0] = 0
        kw["act"] = ACT_RELU if "relu" in f else next((a for n, a in ACT_FLAGS.items() if n in f), ACT_NONE)
        dropout(f, kw)
        L["inp"], kw["in_coff"] = _window(_sparse_ints(g, (ipe if shared else N, H, W, cin), cin * ks * ks), win)
        L["out_init"], kw["out_coff"] = _out_buffer((N, Ho, Wo), cout, win)
        L["kw"] = kw
        out["f"] = L

    d = fl["d"]
    if d is not None:
        assert not d - MLP_FLAGS - {"bias", "drelu", "win"}, d
        win = "win" in d
        K = cout * ks * ks // (1 if stride == 1 else 4 if ks == 3 else 1)
        L = {"w": _dyadic(g, (E, cin, cout, ks, ks)), "bias": None, "res": None, "bn_coef": None, "res_is_out": False}
        kw = dict(cin=cout, cout=cin, ipe=ipe, ks=ks, stride=1, pad=ks - 1 - pad, dtype=dtype, dilate=stride == 2, stats=False)
        kw["res_mode"] = RES_DRELU if "drelu" in d else next(m for n, m in DMODE_FLAGS.items() if n in d)
        dropout(d, kw)
        if "bias" in d:
            L["bias"] = _dyadic(g, (E, cin))
        L["inp"], kw["in_coff"] = _window(_sparse_ints(g, (N, Ho, Wo, cout), K), win)
        L["out_init"], kw["out_coff"] = _out_buffer((N, H, W), cin, win)
        y, L["saved_z"] = saved_output(g, (N, H, W, cin), kw["res_mode"], kw.get("drop_p", 0.0), kw.get("seed", 0), dtype)
        L["res"], kw["res_coff"] = _window(y, win, 48, 32)
        L["kw"] = kw
        out["d"] = L
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# e4m3 operands

def qdq_act(x, in_scale=IN_SCALE):
    """the policy's activation quantiser on float64 values (NaN, the outside of a channel window, stays NaN)"""
    return P.qdq_act(x.to(F32), in_scale).to(F64)


def qdq_weight(w):
    """the policy's weight quantiser, expert by expert: w [E, cout, cin, ks, ks]"""
    return torch.stack([P.qdq_weight(we.to(F32)) for we in w]).to(F64)


def operands(L):
    """(inp, w) as the kernel's arithmetic sees them: the launch's own, or -- e4m3 operands -- what the two quantisers of
    oracle/fp8_policy.py make of them"""
    if not L.get("f8"):
        return L["inp"], L["w"]
    return qdq_act(L["inp"], L["in_scale"]), qdq_weight(L["w"])


def e4m3_operands(L, coutp):
    """the operands of an e4m3 launch from the reference's own statement: weight bytes [E, coutp, taps, cin] =
    e4m3(w / row_scale) with zero pad rows, out_scale [E, coutp] = row_scale / in_scale with NaN in [cout, coutp) (the kernels
    must not read it) and -- a8 -- the input bytes e4m3(x * in_scale) with 0x7f, the e4m3 NaN, outside the channel window
    (None: the input stays bfloat16)"""
    kw, w, s_in = L["kw"], L["w"], L["in_scale"]
    E, cout, cin, ks, _ = w.shape
    wb = torch.zeros(E, coutp, ks * ks, cin, dtype=torch.uint8)
    osc = torch.full((E, coutp), float("nan"), dtype=F32)
    for e in range(E):
        rs = P.row_scale(w[e].to(F32))
        wb[e, :cout] = P.e4m3_bytes((w[e].to(F32) / rs.view(-1, 1, 1, 1))).reshape(cout, cin, ks * ks).permute(0, 2, 1)
        osc[e, :cout] = rs / s_in
    xb = None
    if L["a8"]:
        c0 = kw["in_coff"]
        xb = torch.full(L["inp"].shape, 0x7f, dtype=torch.uint8)
        xb[..., c0:c0 + cin] = P.e4m3_bytes(L["inp"][..., c0:c0 + cin].to(F32) * s_in)
    return wb, osc, xb


def e4m3_values():
    """the 127 non-negative finite e4m3 values, ascending: byte codes 0x00 .. 0x7e (seven subnormals k 2^-9, then 2^e (1 + m / 8)
    up to 448)"""
    return torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).to(F64)


def bf16_neighbour(t, d):
    """the bfloat16 value d steps above (d > 0) or below a positive bfloat16 value"""
    return (t.to(BF16).view(torch.int16) + d).view(BF16).to(F64)


def select_values(a8):
    """the inputs of the select kind TIMES in_scale, every one exact in bfloat16.  a8: the 254 non-NaN byte codes.  bfloat16 input
    (the converting loaders): both signs of
      every e4m3 value, the seven subnormals and the zero (so -0 too) among them;
      every exact tie -- the midpoint of two neighbouring e4m3 values, normal and subnormal, 2^-10 between 0 and the smallest
      subnormal among them -- and its two bfloat16 neighbours;
      values below half the smallest subnormal (they convert to zero);
      values beyond 448 up to 1e4 x 16 (they saturate to 448; 464, halfway to the 480 that e4m3fn does not have, among them)"""
    if a8:
        return torch.cat([torch.arange(0, 127), torch.arange(128, 255)]).to(torch.uint8).view(torch.float8_e4m3fn).to(F64)
    v = e4m3_values()
    ties = (v[:-1] + v[1:]) / 2
    small = torch.tensor([2.0 ** -11, 2.0 ** -14, 2.0 ** -20, 3 * 2.0 ** -12], dtype=F64)
    big = round_to(torch.tensor([450.0, 464.0, 466.0, 480.0, 512.0, 1000.0, 65536.0, 1e4 * 16], dtype=F64), BF16)
    pos = torch.cat([v, ties, bf16_neighbour(ties, 1), bf16_neighbour(ties, -1), small, big])
    return torch.cat([pos, -pos])


def _select_input(g, shape, a8, in_scale):
    """select_values / in_scale, each value as often as any other, in random order"""
    vals = select_values(a8) / in_scale
    n = 1
    for d in shape:
        n *= d
    assert n >= len(vals), (shape, len(vals))
    return vals[torch.arange(n) % len(vals)][torch.randperm(n, generator=g)].reshape(shape)


def _select_weights(g, E, cout, cin, ks):
    """one non-zero per output channel: +-2^j, j in -2 .. 2, at a random input channel; the taps in turn from a random first one,
    so that every tap is some channel's.  Channel 0 of every expert takes the LAST input channel at the left tap of the middle
    filter row: the element the kslice and tapshift mutants get wrong"""
    w = torch.zeros(E, cout, cin * ks * ks, dtype=F64)
    tap = (torch.arange(cout) + torch.randint(0, ks * ks, (E, 1), generator=g)) % (ks * ks)
    at = torch.randint(0, cin, (E, cout), generator=g) * (ks * ks) + tap
    at[:, 0] = (cin - 1) * ks * ks + (ks // 2) * ks
    val = torch.ldexp(torch.ones(E, cout, dtype=F64), torch.randint(-2, 3, (E, cout), generator=g)) * (2 * torch.randint(0, 2, (E, cout), generator=g) - 1)
    w.scatter_(2, at[..., None], val[..., None])
    return w.reshape(E, cout, cin, ks, ks)


@functools.lru_cache(maxsize=4)
def launches(case, kind):
    """{"f" | "d" | "w": launch}: the tensors (float64 values representable in the case's storage type) and keywords of the three
    launches of a case.  A conv launch: inp, w (logical, the launch's own orientation), out_init, bias, res, bn_coef and ``kw``
    (the keywords of conv_ref.conv2d = those of ops.conv2d, but for the tensors); ``res_is_out``: the residual IS the output
    buffer.  A weight-gradient launch: x, dy, bn and ``kw``."""
    assert kind in kinds_of(case), (kind, case_id(case))
    if kind == DYADIC:
        return _dyadic_launches(case)
    E, ipe, cin, cout, H, W, ks, stride, dtype = case[:9]
    fl = flags(case)
    # the select kind: its own weights and input; bias and side input small integers (every float32 sum of the tail stays exact)
    sel = kind == SELECT
    side = "lattice" if sel else kind
    assert not sel or (fl["d"] is None and fl["w"] is None), "a case with e4m3 operands is a forward launch alone"
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(case_id(case) + kind)))
    N, pad = E * ipe, ks // 2
    Ho, Wo = out_size(H, ks, stride, pad), out_size(W, ks, stride, pad)
    out = {}
    # (a stride-2 data gradient: its four parity classes see 1, 2, 2 and 4 of the 9 taps; 1x1: the even pixels see one)
    Rf, Rd = value_range(kind, cin * ks * ks), value_range(kind, cout * ks * ks // (1 if stride == 1 else 4 if ks == 3 else 1))

    f = fl["f"]
    if f is not None:
        shared, win = "shared" in f, "win" in f
        nin = ipe if shared else N
        f8, a8 = bool(f & F8_FLAGS), "a8" in f
        in_scale = next((v for n, v in SCALE_FLAGS.items() if n in f), IN_SCALE)
        assert f8 or (not sel and not f & set(SCALE_FLAGS)), case
        w = _select_weights(g, E, cout, cin, ks) if sel else _ints(g, (E, cout, cin, ks, ks), Rf, kind)
        L = {"w": w, "bias": None, "res": None, "bn_coef": None, "res_is_out": False, "f8": f8, "a8": a8, "in_scale": in_scale}
        kw = dict(cin=cin, cout=cout, ipe=ipe, ks=ks, stride=stride, pad=pad, dtype=dtype, in_shared=shared)
        Rs = 3 if sel else Rf
        if "inbn" in f:
            coef = bn_coefficients(g, E, cin, kind)
            x = planted_z(g, (nin, H, W, cin), coef, ipe, kind)
            L["bn_coef"] = coef
            kw.update(res_mode=RES_INBN, bn_ipe=ipe)
        elif sel:
            x = _select_input(g, (nin, H, W, cin), a8, in_scale)
        else:
            x = _ints(g, (nin, H, W, cin), Rf, kind)
        if "relu" in f and sel:
            kw["act"] = ACT_RELU
        elif "relu" in f:
            # one pixel of image 0 sees a single non-zero input element: with bias[c] = -w[c, 0, centre] + {0, 1, -1} its
            # pre-activations are exactly on the ReLU edge and one step either side, channel by channel
            py, px = min(2, H - 1), min(2, W - 1)
            x[0, max(py - 2, 0):py + 3, max(px - 2, 0):px + 3] = 0
            x[0, py, px, 0] = 1
            kw["act"] = ACT_RELU
        if "bias" in f:
            b = _ints(g, (E, cout), max(Rs, 3), side)
            if "relu" in f and not sel:
                b[0] = -w[0, :, 0, ks // 2, ks // 2] + (torch.arange(cout) % 3 - 1).to(F64)
            L["bias"] = b
        L["inp"], kw["in_coff"] = _window(x, win)
        if "shuf" in f:
            c_up = cout // 4
            kw["shuffle_c"] = c_up
            L["out_init"], kw["out_coff"] = torch.full((N, 2 * Ho, 2 * Wo, 2 * c_up), SENTINEL, dtype=F64), c_up
        else:
            L["out_init"], kw["out_coff"] = _out_buffer((N, Ho, Wo), cout, win)
        if "addin" in f:
            prev = _ints(g, (N, Ho, Wo, cout), 8 * max(Rs, 2), side)
            L["out_init"][..., kw["out_coff"]:kw["out_coff"] + cout] = prev
            kw.update(res_mode=RES_ADD, res_coff=kw["out_coff"])
            L["res_is_out"] = True
        if "add" in f:
            res = _ints(g, (N, Ho, Wo, cout), 8 * max(Rs, 2), side)
            if "relu" in f:
                res[0, min(2, H - 1) // stride, min(2, W - 1) // stride] = 0          # the planted pixel stays on the ReLU edge
            L["res"], kw["res_coff"] = _window(res, win, 48, 32)
            kw["res_mode"] = RES_ADD
        if "drelu" in f:
            L["res"], kw["res_coff"] = _window(_ints(g, (N, Ho, Wo, cout), 2, "lattice"), win, 48, 32)  # the saved output: -2 .. 2
            kw["res_mode"] = RES_DRELU
        kw["stats"] = "stats" in f
        L["kw"] = kw
        out["f"] = L

    d = fl["d"]
    if d is not None:
        # the data gradient of the layer: reads dy [N, Ho, Wo, cout], writes dx [N, H, W, cin]; stride 2: the zero-dilated form
        win, pimg = "win" in d, "pimg" in d
        Ed, ipd = (N, 1) if pimg else (E, ipe)
        w = _ints(g, (Ed, cin, cout, ks, ks), Rd, kind)
        dy = _ints(g, (N, Ho, Wo, cout), Rd, kind)
        L = {"w": w, "bias": None, "res": None, "bn_coef": None, "res_is_out": False}
        kw = dict(cin=cout, cout=cin, ipe=ipd, ks=ks, stride=1, pad=ks - 1 - pad, dtype=dtype, dilate=stride == 2)
        L["inp"], kw["in_coff"] = _window(dy, win)
        prev = None
        if "addin" in d:
            prev = _ints(g, (N, H, W, cin), 8 * max(Rd, 2), kind)
            kw["res_mode"], L["res_is_out"] = RES_ADD, True
        L["out_init"], kw["out_coff"] = _out_buffer((N, H, W), cin, win, prev)
        if "addin" in d:
            kw["res_coff"] = kw["out_coff"]
        if "add" in d:
            L["res"], kw["res_coff"] = _window(_ints(g, (N, H, W, cin), 8 * max(Rd, 2), kind), win, 48, 32)
            kw["res_mode"] = RES_ADD
        if "drelu" in d:
            L["res"], kw["res_coff"] = _window(_ints(g, (N, H, W, cin), 2, "lattice"), win, 48, 32)     # the saved output: -2 .. 2
            kw["res_mode"] = RES_DRELU
        if "dbn" in d:
            coef = bn_coefficients(g, E, cin, kind)
            L["bn_coef"] = coef
            L["res"], kw["res_coff"] = _window(planted_z(g, (N, H, W, cin), coef, ipe, kind), win, 48, 32)
            kw.update(res_mode=RES_DBN, bn_ipe=ipe, stats=True)
        if "bias" in d:
            L["bias"] = _ints(g, (Ed, cin), max(Rd, 3), kind)
        kw.setdefault("stats", False)
        L["kw"] = kw
        out["d"] = L

    wf = fl["w"]
    if wf is not None:
        win, shared, pimg = "win" in wf, "shared" in wf, "pimg" in wf
        ckw = 64 if dtype == BF16 else 32
        Rw = value_range(kind, 144)                                # (the reduction runs over pixels: +-7 whatever the channels)
        x = _ints(g, (ipe if shared else N, H, W, cin), Rw, kind)
        kw = dict(cin=cin, cout=cout, cinp=(cin + ckw - 1) // ckw * ckw, coutp=(cout + ckw - 1) // ckw * ckw, ipe=ipe, ks=ks,
                  stride=stride, pad=pad, dtype=dtype, x_shared=shared, per_image=pimg)
        L = {"bn": None}
        if "bn" in wf:
            # g: a masked gradient (zeros where the mask cleared it); z and the constants on bn_ref's lattice but for c1, a
            # multiple of 1/1024: dz = g A + ((z - mean) Bx + K) is a multiple of 2^-11 below 16 -- exact in float32, and its
            # bfloat16 rounding really rounds; x stays within +-3 so that the sums of x dz are exact too
            x = _ints(g, x.shape, 3, kind)
            coef = bn_coefficients(g, E, cout, "lattice")
            z = torch.randint(-8, 9, (N, Ho, Wo, cout), generator=g).to(F64) / 4
            dy = torch.randint(-6, 7, (N, Ho, Wo, cout), generator=g).to(F64) / 4 * (torch.rand(N, Ho, Wo, cout, generator=g) < 0.6)
            c1 = torch.randint(-512, 513, (E, cout), generator=g).to(F64) / 1024
            c2 = torch.tensor([-1.0, -0.5, 0.5, 1.0], dtype=F64)[torch.randint(0, 4, (E, cout), generator=g)]
            L["bn"] = (z, coef, c1, c2)
        else:
            dy = _ints(g, (N, Ho, Wo, cout), Rw, kind)
        L["x"], kw["x_coff"] = _window(x, win)
        L["dy"], kw["dy_coff"] = _window(dy, win, 48, 32)
        L["kw"] = kw
        out["w"] = L
    return out


def conv_reference(L, rounding="once", mut=""):
    """conv2d of a launch of ``launches``"""
    res = L["out_init"] if L["res_is_out"] else L["res"]
    inp, w = operands(L)
    return conv2d(inp, w, L["out_init"], bias=L["bias"], res=res, bn_coef=L["bn_coef"], rounding=rounding, mut=mut, **L["kw"])


def stored_interval(ref, dtype):
    """(lo, hi) of the stored window: a float32 value within ``allow`` of the reference's rounds into [round(pre - allow),
    round(pre + allow)] -- rounding is monotonic -- which is one value wherever both ends round alike.  float32 storage:
    pre -+ allow itself."""
    if dtype == F32:
        return ref["pre"] - ref["allow"], ref["pre"] + ref["allow"]
    return round_to(ref["pre"] - ref["allow"], dtype), round_to(ref["pre"] + ref["allow"], dtype)


def wgrad_reference(L, evaluate=F64):
    return wgrad(L["x"], L["dy"], bn=L["bn"], evaluate=evaluate, **L["kw"])


def abs_bound(L):
    """max over the output elements of sum |x||w| (+ |bias| + |res|): below 2^24 every float32 partial sum is exact"""
    kw = L["kw"]
    inp, w = operands(L)
    xw = inp[..., kw["in_coff"]:kw["in_coff"] + kw["cin"]]
    if kw.get("res_mode") == RES_INBN:
        c = L["bn_coef"]
        xw = bn_ref.bn_apply(xw, None, c[2], c[3], c[0], c.shape[1], True, kw["dtype"])["y"]
    ho, wo = L["out_init"].shape[1:3]
    if kw.get("shuffle_c"):
        ho, wo = ho // 2, wo // 2
    a = conv_acc(xw.abs(), w.abs(), ipe=kw["ipe"], in_shared=kw.get("in_shared", False), stride=kw["stride"], pad=kw["pad"],
                 ho=ho, wo=wo, dilate=kw.get("dilate", False))
    if L["bias"] is not None:
        a = a + L["bias"].abs().repeat_interleave(kw["ipe"], 0)[:, None, None, :]
    if kw.get("res_mode") == RES_ADD:
        res = L["out_init"] if L["res_is_out"] else L["res"]
        a = a + res[..., kw["res_coff"]:kw["res_coff"] + kw["cout"]].abs()
    return a.max().item()


# ---------------------------------------------------------------------------------------------------------------------------------
# pmoe_mlp_wgrad (csrc/gemm_skinny.hip, mlp_wgrad_kernel): weight and bias gradient of a Linear layer of all experts

WGRAD_MUTANTS = ("bias64",       # the bias gradient summed over the first 64 rows only
                 "padleak")      # the first pad channel of x added into the last real input column of grads


def mlp_wgrad(x, dy, *, cin, cout, cin_real, cout_real, ipe, x_shared=False, x_coff=0, dy_coff=0, evaluate=F64, reverse=False, mut=""):
    """x [Nx, x_ld], dy [N, dy_ld] -> grads [E, cout_real, cin_real], bias_grads [E, cout_real] as include/pmoe_hip.h states them:
    grads[e][o][i] = sum_m dy[e ipe + m][dy_coff + o] x[(x_shared ? m : e ipe + m)][x_coff + i], bias_grads[e][o] = sum_m dy[...].
    Evaluated in ``evaluate``, row by row (``reverse``: from the last row down -- another summation order)"""
    E = dy.shape[0] // ipe
    g = dy[:, dy_coff:dy_coff + cout_real].to(evaluate).reshape(E, ipe, cout_real)
    xs = x[:, x_coff:x_coff + cin_real].to(evaluate)
    xs = xs[None].expand(E, ipe, cin_real) if x_shared else xs.reshape(E, ipe, cin_real)
    assert not torch.isnan(g).any() and not torch.isnan(xs).any()
    grads, bias = torch.zeros(E, cout_real, cin_real, dtype=evaluate), torch.zeros(E, cout_real, dtype=evaluate)
    for m in (reversed(range(ipe)) if reverse else range(ipe)):
        grads = grads + g[:, m, :, None] * xs[:, m, None, :]
        if mut != "bias64" or m < 64:
            bias = bias + g[:, m]
    if mut == "padleak" and cin_real < cin:
        xp = x[:, x_coff + cin_real].to(evaluate)
        xp = xp[None].expand(E, ipe) if x_shared else xp.reshape(E, ipe)
        grads[:, :, -1] += torch.einsum("emo,em->eo", g, xp)
    return {"grads": grads, "bias_grads": bias}


# (E, ipe, cin, cin_real, cout, cout_real, x_shared, x_coff, dy_coff): one row, one input tile; a shared input with one real
# input column; whole 64 x 64 x 64 tiles; a second row chunk of ONE row and ragged tiles in both directions; three row chunks on
# channel windows
MLP_WGRAD_CASES = [
    (2, 1, 8, 8, 8, 8, False, 0, 0),
    (2, 7, 16, 1, 16, 5, True, 0, 0),
    (3, 64, 64, 64, 64, 64, False, 0, 0),
    (1, 65, 72, 70, 136, 130, False, 0, 0),
    (2, 130, 96, 90, 80, 72, False, 16, 32),
]
PAD_FILL = 2.0 ** 60            # the staged pad channels [cin_real, cin) and [cout_real, cout): large and finite (130 products of
#                                 two of them still are), so that one leaking into an output cannot hide
GUARD = 8                       # sentinel elements past the end of grads and bias_grads


@functools.lru_cache(maxsize=None)
def mlp_wgrad_data(case, kind):
    """x, dy (float64 values exact in bfloat16) and the keywords of mlp_wgrad: +-7 integers (unit: {-1, 0, 1}) -- at most 130 rows,
    so every float32 sum is exact in any order; NaN outside the channel windows, PAD_FILL in the pad channels"""
    E, ipe, cin, cin_real, cout, cout_real, shared, xc, dc = case
    g = torch.Generator().manual_seed(sum((i + 1) * int(v) for i, v in enumerate(case)) + len(kind))

    def rows(n, c, c_real, coff):
        t = torch.full((n, coff + c + (8 if coff else 0)), float("nan"), dtype=F64)
        t[:, coff:coff + c] = PAD_FILL * (2 * torch.randint(0, 2, (n, c), generator=g) - 1)
        t[:, coff:coff + c_real] = _ints(g, (n, c_real), 7, kind)
        return t
    kw = dict(cin=cin, cout=cout, cin_real=cin_real, cout_real=cout_real, ipe=ipe, x_shared=shared, x_coff=xc, dy_coff=dc)
    return {"x": rows(ipe if shared else E * ipe, cin, cin_real, xc), "dy": rows(E * ipe, cout, cout_real, dc), "kw": kw}
