// The two ends of the agent's step (pmoe_amd/infer.py:AgentStep; autoagents/image_agent.py:114-125,127-160) around the policy tick:
// the camera's BGRA bytes -> Crop -> Resize -> ToTensor -> the frame history, in one launch, and the sampled action -> the three
// numbers of a carla.VehicleControl.
#include "common.h"

static constexpr int PREC = 32 - 8 - 2;            // Pillow's PRECISION_BITS (csrc/preprocess.hip)
static constexpr int SENSOR_LDS_MAX = 64 * 1024;   // what a launch gets without an opt-in
// A frame is a few dozen tiles: the launch is one tile's latency, so a workgroup is as wide as it can be (1024 threads: 11.7 us at
// the agent's shape against 27.3 with 256)
static constexpr int SENSOR_THREADS = 1024;

__device__ __forceinline__ int clip8(int v) {
    v >>= PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bgra [B][H0][W0][4] bytes (B, G, R, A) -> ring f32 [B][T][3][Hout][Wout], slot T-1 = ToTensor(Resize(Crop(frame))) in R, G, B
// order, the older slots moved down by one; nhwc != NULL: ET [B][Hout][Wout][Cp] of the new frame, zero padded.
// Workgroup (blockIdx.x, blockIdx.y) owns output rows y0 .. y0 + tile_rows - 1 of image blockIdx.y.  Pillow's two integer passes
// (csrc/preprocess.hip: 22-bit coefficients, 8-bit intermediate) with the intermediate in LDS instead of HBM:
//   1. horizontal pass over the cropped source rows s0 .. s0 + span - 1 that the tile's output rows read (s0 = the first output
//      row's first tap, span <= tile_in_rows): one thread per (row, output column) reads whole pixels as dwords -- neighbouring
//      lanes read neighbouring pixels of one row -- and stores its three 8-bit results into stage[row][channel][column];
//   2. barrier;
//   3. vertical pass from LDS, one thread per (output row, column): neighbouring lanes read neighbouring bytes of a staged row.
//      The thread owns its element offset in all T slots of the ring (walked oldest first, like history_push_kernel: nothing
//      reads what another thread writes) and the pixel's NHWC vectors.
// The bound tables are device data nobody has checked: every tap is clamped to the source columns, to the staged rows and to the
// coefficient row, so a wrong table gives wrong pixels, never an access outside stage[], the frame or the tables' rows.
template <typename ET>
__global__ void __launch_bounds__(SENSOR_THREADS)
sensor_push_kernel(const uint32_t* __restrict__ bgra, float* ring, int T, int H0, int W0, int row0, int rows, int Hout, int Wout,
                   const int32_t* __restrict__ hbounds, const int32_t* __restrict__ hk, int hksize,
                   const int32_t* __restrict__ vbounds, const int32_t* __restrict__ vk, int vksize, int tile_rows, int tile_in_rows,
                   ET* __restrict__ nhwc, int Cp) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    const int b = blockIdx.y;
    const int y0 = blockIdx.x * tile_rows;
    const int ny = min(tile_rows, Hout - y0);
    const int s0 = clampi(vbounds[2 * y0], 0, rows - 1);
    const int span = min(tile_in_rows, rows - s0);                       // >= 1
    const uint32_t* img = bgra + ((size_t)b * H0 + row0 + s0) * W0;

    for (int i = threadIdx.x; i < span * Wout; i += SENSOR_THREADS) {
        const int r = i / Wout, xx = i - r * Wout;
        const int xmin = clampi(hbounds[2 * xx], 0, W0 - 1);
        const int cnt = clampi(hbounds[2 * xx + 1], 0, min(hksize, W0 - xmin));
        const uint32_t* p = img + (size_t)r * W0 + xmin;
        const int32_t* k = hk + (size_t)xx * hksize;
        int s2 = 1 << (PREC - 1), s1 = s2, sb = s2;                      // red, green, blue
        for (int x = 0; x < cnt; ++x) {
            const uint32_t px = p[x];
            const int w = k[x];
            sb += (int)(px & 0xffu) * w;
            s1 += (int)((px >> 8) & 0xffu) * w;
            s2 += (int)((px >> 16) & 0xffu) * w;
        }
        uint8_t* o = stage + (size_t)r * 3 * Wout + xx;
        o[0] = (uint8_t)clip8(s2);
        o[Wout] = (uint8_t)clip8(s1);
        o[2 * Wout] = (uint8_t)clip8(sb);
    }
    __syncthreads();

    const size_t HW = (size_t)Hout * Wout;
    for (int i = threadIdx.x; i < ny * Wout; i += SENSOR_THREADS) {
        const int ty = i / Wout, xx = i - ty * Wout;
        const int yy = y0 + ty;
        const int l0 = clampi(vbounds[2 * yy] - s0, 0, span - 1);
        const int cnt = clampi(vbounds[2 * yy + 1], 0, min(vksize, span - l0));
        const int32_t* k = vk + (size_t)yy * vksize;
        const uint8_t* p = stage + (size_t)l0 * 3 * Wout + xx;
        int ss[3] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
        for (int y = 0; y < cnt; ++y, p += 3 * Wout) {
            const int w = k[y];
            ss[0] += (int)p[0] * w;
            ss[1] += (int)p[Wout] * w;
            ss[2] += (int)p[2 * Wout] * w;
        }
        float f[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f[c] = (float)(uint8_t)clip8(ss[c]) / 255.0f;                // ToTensor (preprocess.hip:px_out<float>)
            float* q = ring + ((size_t)b * T * 3 + c) * HW + (size_t)yy * Wout + xx;
            for (int t = 0; t + 1 < T; ++t, q += 3 * HW) *q = q[3 * HW];
            *q = f[c];
        }
        if (nhwc != nullptr) {
            constexpr int VE = 16 / (int)sizeof(ET);
            ET* dst = nhwc + ((size_t)b * HW + (size_t)yy * Wout + xx) * Cp;
            for (int c0 = 0; c0 < Cp; c0 += VE) {
                float v[VE];
#pragma unroll
                for (int j = 0; j < VE; ++j) v[j] = c0 + j < 3 ? f[(c0 + j) % 3] : 0.f;
                stg16(dst + c0, pack16<ET>(v));
            }
        }
    }
}

// image_agent.py:114-125 (postprocess) on the device: actions [B][2] f32 -> control [B][3] f64 = (steer, throttle, brake).  The
// comparisons that pick a branch or a bound are f32 and written so that a NaN falls through them; the throttle floor is the
// DOUBLE 0.4 of the reference, compared in double.
__device__ __forceinline__ float clipf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void __launch_bounds__(256) control_kernel(const float* __restrict__ actions, double* __restrict__ control, int B) {
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        const float a0 = actions[2 * b], a1 = actions[2 * b + 1];
        double steer = 0.0, throttle = 0.0, brake = 0.0;
        if (a1 < -0.5f) {
            brake = (double)clipf(-a1, 0.f, 1.f);
        } else {
            steer = (double)clipf(a0, -1.f, 1.f);
            const double t = (double)clipf(a1, 0.f, 0.75f);
            throttle = 0.4 > t ? 0.4 : t;
        }
        control[3 * b] = steer;
        control[3 * b + 1] = throttle;
        control[3 * b + 2] = brake;
    }
}

extern "C" {

int pmoe_sensor_push(const uint8_t* bgra, void* ring, int32_t B, int32_t T, int32_t H0, int32_t W0, int32_t row0, int32_t rows,
                     int32_t Hout, int32_t Wout, const int32_t* hbounds, const int32_t* hcoeffs, int32_t hksize,
                     const int32_t* vbounds, const int32_t* vcoeffs, int32_t vksize, int32_t tile_rows, int32_t tile_in_rows,
                     void* nhwc, int32_t Cp, int32_t nhwc_dtype, void* stream) {
    if (!bgra || !ring || !hbounds || !hcoeffs || !vbounds || !vcoeffs || (uintptr_t)bgra % 4 || (uintptr_t)ring % 4)
        return PMOE_ERR_ARG;
    if (B < 1 || B > 65535 || T < 1 || H0 < 1 || W0 < 1 || rows < 1 || Hout < 1 || Wout < 1 || hksize < 1 || vksize < 1 ||
        tile_in_rows < 1)
        return PMOE_ERR_ARG;
    if (row0 < 0 || row0 > H0 - rows) return PMOE_ERR_ARG;                        // the crop lies inside the frame
    if (tile_rows != 8 && tile_rows != 4 && tile_rows != 2 && tile_rows != 1) return PMOE_ERR_ARG;
    // the NHWC copy: the rules of pmoe_history_push for an item of 3 channel planes
    if (nhwc && (Cp < 3 || (uintptr_t)nhwc % 16 || (nhwc_dtype != PMOE_DT_F32 && nhwc_dtype != PMOE_DT_BF16) ||
                 Cp % (nhwc_dtype == PMOE_DT_F32 ? 4 : 8)))
        return PMOE_ERR_ARG;
    const long long lds = (long long)tile_in_rows * Wout * 3;
    if (lds > SENSOR_LDS_MAX) return PMOE_ERR_UNSUPPORTED;
    const int tiles = (Hout + tile_rows - 1) / tile_rows;
    const dim3 grid(grid_for((long long)tiles * 256, INT_MAX), B);                // = tiles: one workgroup per tile and image
    const uint32_t* px = reinterpret_cast<const uint32_t*>(bgra);
    const dim3 block(SENSOR_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    if (nhwc && nhwc_dtype == PMOE_DT_BF16)
        return launch<sensor_push_kernel<bf16>, 0>(grid, block, (size_t)lds, st, px, (float*)ring, T, H0, W0, row0, rows, Hout, Wout,
                                                   hbounds, hcoeffs, hksize, vbounds, vcoeffs, vksize, tile_rows, tile_in_rows,
                                                   (bf16*)nhwc, Cp);
    return launch<sensor_push_kernel<float>, 0>(grid, block, (size_t)lds, st, px, (float*)ring, T, H0, W0, row0, rows, Hout, Wout,
                                                hbounds, hcoeffs, hksize, vbounds, vcoeffs, vksize, tile_rows, tile_in_rows,
                                                (float*)nhwc, Cp);
}

int pmoe_control_postprocess(const float* actions, double* control, int32_t B, void* stream) {
    if (!actions || !control || B < 1) return PMOE_ERR_ARG;
    return launch<control_kernel, 0>(dim3(grid_for(B, 64)), dim3(256), 0, (hipStream_t)stream, actions, control, B);
}

}  // extern "C"
