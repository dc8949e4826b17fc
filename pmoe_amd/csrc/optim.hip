// Fused optimizer tail of the stage-2 step (reference trainer/train_2.py:157-165,184):
//   clip_grad_norm_(params, max_norm)  ->  global L2 norm over ~620 gradient tensors + one scale
//   Adam(amsgrad=True).step()          ->  one multi-tensor update (optionally also writing the engine's packed operands)
//   RMSprop(centered=True).step()      ->  the same launch with the other update rule (train_2.py:62-73 `optimizer: rmsprop`)
//   AveragedModel.update_parameters()  ->  one multi-tensor running mean
// The reference issues a handful of launches (and a .item() sync) PER parameter tensor; here each stage is one launch
// over a chunk table: tensor t is cut into chunks of PMOE_OPT_CHUNK elements, workgroup i handles chunk
// (chunk_tensor[i], chunk_index[i]).  All of it is HBM-bound streaming work: 16-byte accesses when the chunk base is
// aligned (always, for torch allocations), scalar tail otherwise.  Nothing synchronises with the host: the clip
// coefficient stays in device memory and is consumed by the Adam kernel.
#include "common.h"

static constexpr int CHUNK = PMOE_OPT_CHUNK;

__device__ __forceinline__ float block_sum(float v, float* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;      // valid in thread 0
}

__global__ void __launch_bounds__(256) mt_sqsum_kernel(const pmoe_opt_tensor* __restrict__ tab,
                                                      const int32_t* __restrict__ chunk_tensor,
                                                      const int32_t* __restrict__ chunk_index,
                                                      float* __restrict__ partial) {
    const pmoe_opt_tensor t = tab[chunk_tensor[blockIdx.x]];
    const long long base = (long long)chunk_index[blockIdx.x] * CHUNK;
    long long n = t.numel - base;
    if (n > CHUNK) n = CHUNK;
    const float* g = t.grad + base;
    float s = 0.f;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const long long nv = n >> 2;
        for (long long i = threadIdx.x; i < nv; i += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + 4 * i);
            s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        }
        for (long long i = (nv << 2) + threadIdx.x; i < n; i += 256) s += g[i] * g[i];
    } else {
        for (long long i = threadIdx.x; i < n; i += 256) s += g[i] * g[i];
    }
    __shared__ float red[4];
    const float tot = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// norm[0] = sqrt(sum partial) ; norm[1] = clip coefficient min(1, max_norm / (norm + 1e-6))  (torch clip_grad_norm_)
__global__ void __launch_bounds__(256) mt_norm_finish_kernel(const float* __restrict__ partial, int n, float max_norm,
                                                            float* __restrict__ norm) {
    double s = 0.0;            // fixed order, double accumulation: deterministic and exact enough for 1e-6 parity
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float nr = (float)sqrt(red[0]);
        norm[0] = nr;
        const float c = max_norm > 0.f ? max_norm / (nr + 1e-6f) : 1.f;
        norm[1] = c < 1.f ? c : 1.f;
    }
}

__global__ void __launch_bounds__(256) mt_scale_kernel(const pmoe_opt_tensor* __restrict__ tab,
                                                      const int32_t* __restrict__ chunk_tensor,
                                                      const int32_t* __restrict__ chunk_index,
                                                      const float* __restrict__ norm) {
    const float c = norm[1];
    if (c >= 1.f) return;
    const pmoe_opt_tensor t = tab[chunk_tensor[blockIdx.x]];
    const long long base = (long long)chunk_index[blockIdx.x] * CHUNK;
    long long n = t.numel - base;
    if (n > CHUNK) n = CHUNK;
    float* g = const_cast<float*>(t.grad) + base;
    for (long long i = threadIdx.x; i < n; i += 256) g[i] *= c;
}

// torch.optim.Adam (single-tensor formulas of torch/optim/adam.py, maximize=False, capturable=False):
//   g' = clip * g (+ wd * p);  m = m + (1-b1)(g' - m);  v = b2 v + (1-b2) g'^2;  vmax = max(vmax, v)
//   p -= (lr / bc1) * m / (sqrt(vmax or v) / sqrt(bc2) + eps)
//
// An update rule (AdamCoef, RmspropCoef) is the coefficients of one launch plus three members: upd(g, p, a, b, x) -> the new
// parameter, with a / b / x the values of the row's exp_avg / exp_avg_sq / max_exp_avg_sq slots, and has_a() / has_x(): whether
// the rule keeps state in the first and the third slot (the second is always live).  A slot that is not live is never
// dereferenced.  Everything below the rules -- the 16-byte run, the chunk walk, the tile walk and the pack stores -- is written
// once, over the rule.
struct AdamCoef {
    float clip, weight_decay, beta1, beta2, eps, step_size, inv_bc2s;
    int amsgrad;
    __device__ __forceinline__ bool has_a() const { return true; }
    __device__ __forceinline__ bool has_x() const { return amsgrad != 0; }
    __device__ __forceinline__ float upd(float gi, float pi, float& mi, float& vi, float& mx) const;
};

// The one place the update is written: mt_adam_kernel and mt_adam_pack_kernel both call it, so that a parameter comes out with
// the same bits whichever launch updates it and wherever in a launch it falls.  The roundings are spelled out and the compiler's
// own contraction is off in here: left to itself it fused the expressions differently in the 16-byte loop and in the scalar
// tail, so an element's last bit depended on the path it took.  The form is the one the 16-byte loop has always had.
__device__ __forceinline__ float adam_upd(const AdamCoef& c, float gi, float pi, float& mi, float& vi, float& mx) {
#pragma clang fp contract(off)
    gi *= c.clip;
    if (c.weight_decay != 0.f) gi = __builtin_fmaf(c.weight_decay, pi, gi);
    mi = __builtin_fmaf(1.f - c.beta1, gi - mi, mi);
    vi = __builtin_fmaf(vi, c.beta2, ((1.f - c.beta2) * gi) * gi);
    float d = vi;
    if (c.amsgrad) {
        mx = fmaxf(mx, vi);
        d = mx;
    }
    return __builtin_fmaf(-c.step_size, mi / __builtin_fmaf(sqrtf(d), c.inv_bc2s, c.eps), pi);
}

__device__ __forceinline__ float AdamCoef::upd(float gi, float pi, float& mi, float& vi, float& mx) const {
    return adam_upd(*this, gi, pi, mi, vi, mx);
}

// bias corrections: one value for all tensors (kernel argument, > 0) or the per-tensor entries of the table
__device__ __forceinline__ AdamCoef adam_coef(const pmoe_opt_tensor& t, float lr, float beta1, float beta2, float eps,
                                              float weight_decay, int amsgrad, float bc1_all, float bc2s_all,
                                              const float* norm) {
    AdamCoef c;
    c.clip = norm ? norm[1] : 1.f;
    c.weight_decay = weight_decay;
    c.beta1 = beta1;
    c.beta2 = beta2;
    c.eps = eps;
    c.step_size = lr / (bc1_all > 0.f ? bc1_all : t.bc1);
    c.inv_bc2s = 1.f / (bc2s_all > 0.f ? bc2s_all : t.bc2_sqrt);
    c.amsgrad = amsgrad;
    return c;
}

// torch.optim.RMSprop (torch/optim/rmsprop.py:_single_tensor_rmsprop, maximize=False); the formula, line by line, is in the
// header at pmoe_mt_rmsprop.  Slots: a = momentum_buffer (momentum > 0), b = square_avg, x = grad_avg (centered).
struct RmspropCoef {
    float clip, weight_decay, alpha, eps, lr, momentum;
    int centered;
    __device__ __forceinline__ bool has_a() const { return momentum > 0.f; }
    __device__ __forceinline__ bool has_x() const { return centered != 0; }
    __device__ __forceinline__ float upd(float gi, float pi, float& buf, float& sa, float& ga) const;
};

// The one place this update is written, like adam_upd and for the same reason: one rounding per line, no contraction.  No
// clamp under the square root: torch has none, and a centered sa - ga^2 that rounds below zero is NaN in both.
__device__ __forceinline__ float rmsprop_upd(const RmspropCoef& c, float gi, float pi, float& buf, float& sa, float& ga) {
#pragma clang fp contract(off)
    gi *= c.clip;
    if (c.weight_decay != 0.f) gi = __builtin_fmaf(c.weight_decay, pi, gi);
    sa = __builtin_fmaf(sa, c.alpha, ((1.f - c.alpha) * gi) * gi);
    float d;
    if (c.centered) {
        ga = __builtin_fmaf(1.f - c.alpha, gi - ga, ga);
        d = sqrtf(__builtin_fmaf(-ga, ga, sa)) + c.eps;
    } else {
        d = sqrtf(sa) + c.eps;
    }
    const float q = gi / d;
    if (c.momentum > 0.f) {
        buf = __builtin_fmaf(buf, c.momentum, q);
        return __builtin_fmaf(-c.lr, buf, pi);
    }
    return __builtin_fmaf(-c.lr, q, pi);
}

__device__ __forceinline__ float RmspropCoef::upd(float gi, float pi, float& buf, float& sa, float& ga) const {
    return rmsprop_upd(*this, gi, pi, buf, sa, ga);
}

__device__ __forceinline__ RmspropCoef rmsprop_coef(float lr, float alpha, float eps, float weight_decay, float momentum,
                                                    int centered, const float* norm) {
    RmspropCoef c;
    c.clip = norm ? norm[1] : 1.f;
    c.weight_decay = weight_decay;
    c.alpha = alpha;
    c.eps = eps;
    c.lr = lr;
    c.momentum = momentum;
    c.centered = centered;
    return c;
}

// n consecutive elements, one thread: 4 as 16-byte accesses (vec: the caller has checked the alignment), fewer one by one.
// a / x are read and written only where the rule has them.  stage != nullptr also leaves the updated parameters there.
template <class R>
__device__ __forceinline__ void opt_run(const R& c, float* p, const float* g, float* a, float* b, float* x, int n, bool vec,
                                        float* stage) {
    const bool ha = c.has_a(), hx = c.has_x();
    if (vec) {
        f32x4 pv = *reinterpret_cast<f32x4*>(p);
        f32x4 bv = *reinterpret_cast<f32x4*>(b);
        f32x4 av = ha ? *reinterpret_cast<f32x4*>(a) : bv;
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g);
        f32x4 xv = hx ? *reinterpret_cast<f32x4*>(x) : bv;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float ai = av[k], bi = bv[k], xi = xv[k];
            pv[k] = c.upd(gv[k], pv[k], ai, bi, xi);
            av[k] = ai; bv[k] = bi; xv[k] = xi;
        }
        *reinterpret_cast<f32x4*>(p) = pv;
        if (ha) *reinterpret_cast<f32x4*>(a) = av;
        *reinterpret_cast<f32x4*>(b) = bv;
        if (hx) *reinterpret_cast<f32x4*>(x) = xv;
        if (stage) {
#pragma unroll
            for (int k = 0; k < 4; ++k) stage[k] = pv[k];
        }
        return;
    }
    for (int i = 0; i < n; ++i) {
        float ai = ha ? a[i] : 0.f, bi = b[i], xi = hx ? x[i] : 0.f;
        const float pn = c.upd(g[i], p[i], ai, bi, xi);
        p[i] = pn;
        if (ha) a[i] = ai;
        b[i] = bi;
        if (hx) x[i] = xi;
        if (stage) stage[i] = pn;
    }
}

// chunk `chunk` of tensor t: 16-byte accesses where param, grad and the live state pointers are all 16-byte aligned, with a
// scalar tail after them; scalar throughout when they are not
template <class R>
__device__ __forceinline__ void opt_chunk(const R& c, const pmoe_opt_tensor& t, int chunk) {
    const long long base = (long long)chunk * CHUNK;
    long long n = t.numel - base;
    if (n > CHUNK) n = CHUNK;
    float* p = t.param + base;
    const float* g = t.grad + base;
    float* a = c.has_a() ? t.exp_avg + base : nullptr;
    float* b = t.exp_avg_sq + base;
    float* x = c.has_x() ? t.max_exp_avg_sq + base : nullptr;
    const bool aligned = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(a) |
                           reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
    long long done = 0;
    if (aligned) {
        const long long nv = n >> 2;
        for (long long i = threadIdx.x; i < nv; i += 256)
            opt_run(c, p + 4 * i, g + 4 * i, a ? a + 4 * i : nullptr, b + 4 * i, x ? x + 4 * i : nullptr, 4, true, nullptr);
        done = nv << 2;
    }
    for (long long i = done + threadIdx.x; i < n; i += 256)
        opt_run(c, p + i, g + i, a ? a + i : nullptr, b + i, x ? x + i : nullptr, 1, false, nullptr);
}

__global__ void __launch_bounds__(256) mt_adam_kernel(const pmoe_opt_tensor* __restrict__ tab,
                                                     const int32_t* __restrict__ chunk_tensor,
                                                     const int32_t* __restrict__ chunk_index, float lr, float beta1,
                                                     float beta2, float eps, float weight_decay, int amsgrad,
                                                     float bc1_all, float bc2s_all, const float* __restrict__ norm) {
    const pmoe_opt_tensor t = tab[chunk_tensor[blockIdx.x]];
    opt_chunk(adam_coef(t, lr, beta1, beta2, eps, weight_decay, amsgrad, bc1_all, bc2s_all, norm), t,
              chunk_index[blockIdx.x]);
}

__global__ void __launch_bounds__(256) mt_rmsprop_kernel(const pmoe_opt_tensor* __restrict__ tab,
                                                        const int32_t* __restrict__ chunk_tensor,
                                                        const int32_t* __restrict__ chunk_index, float lr, float alpha,
                                                        float eps, float weight_decay, float momentum, int centered,
                                                        const float* __restrict__ norm) {
    const pmoe_opt_tensor t = tab[chunk_tensor[blockIdx.x]];
    opt_chunk(rmsprop_coef(lr, alpha, eps, weight_decay, momentum, centered, norm), t, chunk_index[blockIdx.x]);
}

// ---- the same updates, leaving the engine's packed operands current (include/pmoe_hip.h: pmoe_mt_adam_packs) ---------------
// A workgroup owns one (co block) x (ci block) x (all taps) tile of one tensor.  In the parameter W[co][ci][tp] a tile row is one
// contiguous run of cols * taps floats, so the update streams it exactly like the chunk walk (16-byte accesses from the first
// 16-byte boundary of each row on) and leaves the new values in LDS; the two operands are then written from LDS in THEIR
// order: fwd [co][tp][ci] with ci across the lanes (runs of cols elements), dgrd [ci][taps-1-tp][co] with co across the lanes
// (runs of rows elements) -- tiles of >= 16 x 16 channels make both runs >= 32 bytes in bf16.  A flat chunk of the parameter
// would instead scatter the dgrd stores as isolated 2-byte writes.  The LDS row stride is odd: the dgrd pass reads a column.
// All offsets are 32-bit (a tensor and one expert's pack are < 2^31 elements, checked by the caller).
template <typename T>
__device__ __forceinline__ void pack_store_tile(const pmoe_opt_pack& k, const float* stage, unsigned rs, unsigned co0,
                                                unsigned ci0, unsigned rows, unsigned cols) {
    const unsigned taps = (unsigned)k.taps;
    const unsigned n = rows * cols * taps;
    if (T* fwd = reinterpret_cast<T*>(k.fwd)) {
        const unsigned row = (unsigned)k.row0 + co0;
        for (unsigned i = threadIdx.x; i < n; i += 256) {
            const unsigned ci = i % cols;
            const unsigned t = i / cols;
            const unsigned tp = t % taps;
            const unsigned r = t / taps;
            fwd[((row + r) * taps + tp) * (unsigned)k.cinp + ci0 + ci] = from_f32<T>(stage[r * rs + ci * taps + tp]);
        }
    }
    if (T* dgrd = reinterpret_cast<T*>(k.dgrd)) {
        const unsigned col = (unsigned)k.col0 + co0;
        for (unsigned i = threadIdx.x; i < n; i += 256) {
            const unsigned r = i % rows;
            const unsigned q = i / rows;           // = ci * taps + tp: the element's place in its LDS row
            const unsigned tp = q % taps;
            const unsigned ci = q / taps;
            dgrd[((ci0 + ci) * taps + (taps - 1 - tp)) * (unsigned)k.dgrd_ld + col + r] = from_f32<T>(stage[r * rs + q]);
        }
    }
}

// the tile (co0, ci0) of tensor t with sink k: update through `stage` (PMOE_OPT_PACK_STAGE floats of LDS), then the pack stores
template <class R>
__device__ __forceinline__ void opt_pack_tile(const R& c, const pmoe_opt_tensor& t, const pmoe_opt_pack& k, int co0, int ci0,
                                              float* stage) {
    if (co0 < 0 || ci0 < 0 || co0 >= k.cout || ci0 >= k.cin || k.taps < 1 || k.tco < 1 || k.tci < 1) return;
    const unsigned rows = (unsigned)min(k.tco, k.cout - co0), cols = (unsigned)min(k.tci, k.cin - ci0);
    const unsigned len = cols * (unsigned)k.taps;              // one tile row: contiguous in the parameter
    const unsigned rs = len | 1u;
    if (rows * rs > (unsigned)PMOE_OPT_PACK_STAGE || (long long)k.cout * k.cin * k.taps != t.numel) return;
    float* a = c.has_a() ? t.exp_avg : nullptr;
    float* x = c.has_x() ? t.max_exp_avg_sq : nullptr;
    const bool aligned = ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
                           reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(t.exp_avg_sq) |
                           reinterpret_cast<uintptr_t>(x)) & 15) == 0;
    const unsigned row_stride = (unsigned)k.cin * (unsigned)k.taps;
    const unsigned s0 = ((unsigned)co0 * (unsigned)k.cin + (unsigned)ci0) * (unsigned)k.taps;
    // work units of a row: unit 0 = the elements before the row's first 16-byte boundary, units 1.. = one 16-byte group each,
    // the last one the (shorter) rest
    const unsigned upr = 1u + ((len + 3u) >> 2);
    for (unsigned u = threadIdx.x; u < rows * upr; u += 256) {
        const unsigned r = u / upr, j = u - r * upr;
        const unsigned s = s0 + r * row_stride;
        unsigned head = aligned ? ((4u - (s & 3u)) & 3u) : len;
        if (head > len) head = len;
        const unsigned nvec = (len - head) >> 2;
        unsigned lo, n;
        bool vec = false;
        if (j == 0) {
            lo = 0; n = head;
        } else if (j - 1 < nvec) {
            lo = head + 4u * (j - 1); n = 4; vec = true;
        } else if (j - 1 == nvec) {
            lo = head + 4u * nvec; n = len - lo;
        } else {
            continue;
        }
        const unsigned o = s + lo;
        opt_run(c, t.param + o, t.grad + o, a ? a + o : nullptr, t.exp_avg_sq + o, x ? x + o : nullptr, (int)n, vec,
                stage + r * rs + lo);
    }
    __syncthreads();
    if (k.dtype == PMOE_DT_BF16)
        pack_store_tile<bf16>(k, stage, rs, (unsigned)co0, (unsigned)ci0, rows, cols);
    else if (k.dtype == PMOE_DT_F32)
        pack_store_tile<float>(k, stage, rs, (unsigned)co0, (unsigned)ci0, rows, cols);
}

__global__ void __launch_bounds__(256) mt_adam_pack_kernel(const pmoe_opt_tensor* __restrict__ tab,
                                                          const pmoe_opt_pack* __restrict__ packs,
                                                          const int32_t* __restrict__ tile_tensor,
                                                          const int32_t* __restrict__ tile_co0,
                                                          const int32_t* __restrict__ tile_ci0, float lr, float beta1,
                                                          float beta2, float eps, float weight_decay, int amsgrad,
                                                          float bc1_all, float bc2s_all, const float* __restrict__ norm) {
    __shared__ float stage[PMOE_OPT_PACK_STAGE];
    const int ti = tile_tensor[blockIdx.x];
    const pmoe_opt_tensor t = tab[ti];
    opt_pack_tile(adam_coef(t, lr, beta1, beta2, eps, weight_decay, amsgrad, bc1_all, bc2s_all, norm), t, packs[ti],
                  tile_co0[blockIdx.x], tile_ci0[blockIdx.x], stage);
}

__global__ void __launch_bounds__(256) mt_rmsprop_pack_kernel(const pmoe_opt_tensor* __restrict__ tab,
                                                             const pmoe_opt_pack* __restrict__ packs,
                                                             const int32_t* __restrict__ tile_tensor,
                                                             const int32_t* __restrict__ tile_co0,
                                                             const int32_t* __restrict__ tile_ci0, float lr, float alpha,
                                                             float eps, float weight_decay, float momentum, int centered,
                                                             const float* __restrict__ norm) {
    __shared__ float stage[PMOE_OPT_PACK_STAGE];
    const int ti = tile_tensor[blockIdx.x];
    opt_pack_tile(rmsprop_coef(lr, alpha, eps, weight_decay, momentum, centered, norm), tab[ti], packs[ti],
                  tile_co0[blockIdx.x], tile_ci0[blockIdx.x], stage);
}

// AveragedModel.update_parameters (torch/optim/swa_utils.py): first call copies, later p_avg += (p - p_avg) / (n + 1)
__global__ void __launch_bounds__(256) mt_swa_kernel(const pmoe_opt_tensor* __restrict__ tab,
                                                    const int32_t* __restrict__ chunk_tensor,
                                                    const int32_t* __restrict__ chunk_index, float inv_np1) {
    const pmoe_opt_tensor t = tab[chunk_tensor[blockIdx.x]];
    const long long base = (long long)chunk_index[blockIdx.x] * CHUNK;
    long long n = t.numel - base;
    if (n > CHUNK) n = CHUNK;
    const float* p = t.param + base;
    float* a = t.swa + base;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const float ai = a[i];
        a[i] = inv_np1 >= 1.f ? p[i] : ai + (p[i] - ai) * inv_np1;
    }
}

extern "C" {

int pmoe_mt_grad_norm(const pmoe_opt_tensor* table, const int32_t* chunk_tensor, const int32_t* chunk_index,
                      int32_t n_chunks, float max_norm, float* partial, float* norm, int32_t scale_grads, void* stream) {
    if (n_chunks < 1 || !table || !partial || !norm) return PMOE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_RET((launch<mt_sqsum_kernel, 0>(dim3(n_chunks), dim3(256), 0, st, table, chunk_tensor, chunk_index, partial)));
    HIP_RET((launch<mt_norm_finish_kernel, 0>(dim3(1), dim3(256), 0, st, partial, n_chunks, max_norm, norm)));
    if (!scale_grads) return 0;
    return launch<mt_scale_kernel, 0>(dim3(n_chunks), dim3(256), 0, st, table, chunk_tensor, chunk_index, norm);
}

int pmoe_mt_adam(const pmoe_opt_tensor* table, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks,
                 float lr, float beta1, float beta2, float eps, float weight_decay, int32_t amsgrad, float bc1_all,
                 float bc2_sqrt_all, const float* norm, void* stream) {
    if (n_chunks < 1 || !table) return PMOE_ERR_ARG;
    return launch<mt_adam_kernel, 0>(dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor, chunk_index, lr, beta1,
                                     beta2, eps, weight_decay, amsgrad, bc1_all, bc2_sqrt_all, norm);
}

int pmoe_mt_adam_packs(const pmoe_opt_tensor* table, const pmoe_opt_pack* packs, const int32_t* tile_tensor,
                       const int32_t* tile_co0, const int32_t* tile_ci0, int32_t n_tiles, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int32_t amsgrad, float bc1_all, float bc2_sqrt_all, const float* norm,
                       void* stream) {
    if (n_tiles < 1 || !table || !packs || !tile_tensor || !tile_co0 || !tile_ci0) return PMOE_ERR_ARG;
    return launch<mt_adam_pack_kernel, 0>(dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, table, packs, tile_tensor, tile_co0,
                                          tile_ci0, lr, beta1, beta2, eps, weight_decay, amsgrad, bc1_all, bc2_sqrt_all, norm);
}

int pmoe_mt_rmsprop(const pmoe_opt_tensor* table, const int32_t* chunk_tensor, const int32_t* chunk_index, int32_t n_chunks,
                    float lr, float alpha, float eps, float weight_decay, float momentum, int32_t centered, const float* norm,
                    void* stream) {
    if (n_chunks < 1 || !table || !chunk_tensor || !chunk_index) return PMOE_ERR_ARG;
    return launch<mt_rmsprop_kernel, 0>(dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor, chunk_index, lr,
                                        alpha, eps, weight_decay, momentum, centered, norm);
}

int pmoe_mt_rmsprop_packs(const pmoe_opt_tensor* table, const pmoe_opt_pack* packs, const int32_t* tile_tensor,
                          const int32_t* tile_co0, const int32_t* tile_ci0, int32_t n_tiles, float lr, float alpha, float eps,
                          float weight_decay, float momentum, int32_t centered, const float* norm, void* stream) {
    if (n_tiles < 1 || !table || !packs || !tile_tensor || !tile_co0 || !tile_ci0) return PMOE_ERR_ARG;
    return launch<mt_rmsprop_pack_kernel, 0>(dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, table, packs, tile_tensor, tile_co0,
                                             tile_ci0, lr, alpha, eps, weight_decay, momentum, centered, norm);
}

int pmoe_mt_swa_update(const pmoe_opt_tensor* table, const int32_t* chunk_tensor, const int32_t* chunk_index,
                       int32_t n_chunks, int64_t n_averaged, void* stream) {
    if (n_chunks < 1 || !table || n_averaged < 0) return PMOE_ERR_ARG;
    return launch<mt_swa_kernel, 0>(dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor, chunk_index,
                                    1.f / (float)(n_averaged + 1));
}

}  // extern "C"
