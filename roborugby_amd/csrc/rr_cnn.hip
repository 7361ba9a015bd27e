// rr_cnn.hip -- the pixel agent's choose_action: the forward of the fixed convolutional Q network (conv 8x8/4 -> conv 4x4/2 -> 256 -> 8,
// roborugby_amd/dqn.py PixelQNetwork) over the planar uint8 frames of PixelObservation, argmax and the epsilon-greedy draw, on the bf16
// matrix cores (v_mfma_f32_16x16x32_bf16).  C-ABI and the arithmetic contract: rr_cnn_act in include/roborugby_amd.h.  Two launches:
//
//   k_cnn_prep   rounds the four weight tensors to bf16 (nearest-even) into the handle's scratch, as they stand at call time
//   k_cnn_act    256 threads (one wavefront per SIMD), persistent over tiles of TM = 32 rows.  Per tile:
//                  conv1 + conv2, one image per wavefront, eight rounds.  A frame (3 channels, 12 KB) goes global -> registers -> the
//                  wavefront's LDS stage as it stands; the next frame's loads are issued before this frame's products.  conv1 is an
//                  implicit GEMM: M = the 225 output positions in 15 tiles of 16 (the last tile's 15 idle rows repeat position 224 and
//                  are dropped), N = the 16 output channels, K = (c, ky, kx) with kx fastest -- a lane's A fragment is 8 adjacent bytes
//                  of one image row (two 4-byte LDS reads), turned into bf16 by cvt_f32_ubyte + the float's upper half (exact).  The 60
//                  accumulator registers stay across the frames of a stack.  Epilogue: 2^-8 scale, bias, ReLU in fp32, bf16 to LDS
//                  ([16][15][16]).  conv2 the same way (M = 36 positions in 3 tiles, N = 32 in 2, K = 256 in torch's (ic, ky, kx)
//                  order: a fragment is two runs of four adjacent activations); its output lands in the tile's [32][1152] bf16 rows.
//                  fc1: M = the tile's 32 rows, every wavefront 64 of the 256 outputs, A from LDS (16-byte reads), the 1152 x 256 bf16
//                  weights stream from L2 (590 KB per tile).  fc2 (8 outputs in one 16-wide tile) on two wavefronts; argmax + draw on
//                  32 lanes.
//                No atomics; no activation goes to HBM; rows >= n are neither read nor written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/roborugby_amd.h"
#include "rr_dqn_shared.hpp"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef __bf16 bf8v __attribute__((ext_vector_type(8)));

constexpr int NA = 8, NT = 256, TM = 32;
constexpr int FRAME_BYTES = 3 * 64 * 64;          // one frame of one row: 3 planar channels
constexpr int H1_IMG = 16 * 15 * 16;              // conv1's output of one image in LDS: [16 channels][15 rows][16: 15 columns + 1]
constexpr int FLAT = 32 * 6 * 6, HID = 256;
constexpr int LDH2 = FLAT + 8, LDH3 = HID + 8;    // LDS row strides (bf16 elements): 16-byte-aligned rows, banks shifted from row to row
constexpr int W2_COUNT = 32 * 16 * 4 * 4, W3_COUNT = HID * FLAT, W4_COUNT = NA * HID;
constexpr int MAX_CHANNELS = 12;
constexpr size_t SCRATCH_ELEMS = (size_t)16 * MAX_CHANNELS * 64 + W2_COUNT + W3_COUNT + W4_COUNT;

struct CnnNet { const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4; };

// fp32 -> bf16, round to nearest, ties to even, on the bit pattern (NaN stays NaN)
__device__ __forceinline__ uint32_t bf16_rne(float x) {
    const uint32_t u = __float_as_uint(x);
    if (x != x) return 0x7FC0u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float relu(float v) { return v > 0.0f ? v : 0.0f; }
__device__ __forceinline__ bf8v as_frag(uint4 v) { return __builtin_bit_cast(bf8v, v); }
__device__ __forceinline__ f4v mfma(uint4 a, uint4 b, f4v c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a), as_frag(b), c, 0, 0, 0); }
// four pixels of one 4-byte word -> four bf16 (two words): the upper half of float(byte) is the byte's value exactly
__device__ __forceinline__ void pixels4(uint32_t w, uint32_t &lo, uint32_t &hi) {
    const uint32_t f0 = __float_as_uint((float)(w & 0xFFu)), f1 = __float_as_uint((float)((w >> 8) & 0xFFu));
    const uint32_t f2 = __float_as_uint((float)((w >> 16) & 0xFFu)), f3 = __float_as_uint((float)(w >> 24));
    lo = (f0 >> 16) | (f1 & 0xFFFF0000u);
    hi = (f2 >> 16) | (f3 & 0xFFFF0000u);
}

__global__ __launch_bounds__(256) void k_cnn_prep(CnnNet net, int w1_count, uint16_t *out) {
    const int total = w1_count + W2_COUNT + W3_COUNT + W4_COUNT;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        float v;
        if (i < w1_count) v = net.w1[i];
        else if (i < w1_count + W2_COUNT) v = net.w2[i - w1_count];
        else if (i < w1_count + W2_COUNT + W3_COUNT) v = net.w3[i - w1_count - W2_COUNT];
        else v = net.w4[i - w1_count - W2_COUNT - W3_COUNT];
        out[i] = (uint16_t)bf16_rne(v);
    }
}

// one frame of row `row` (12 KB, contiguous) into 12 registers per lane; zeros for a row past the end
__device__ __forceinline__ void load_frame(uint4 pre[12], const uint8_t *pixels, int row, int n, int channels, int frame, int lane) {
    if (row < n) {
        const uint4 *src = reinterpret_cast<const uint4 *>(pixels + ((size_t)row * channels + 3 * frame) * 4096);
#pragma unroll
        for (int i = 0; i < 12; i++) pre[i] = src[i * 64 + lane];
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) pre[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

__global__ __launch_bounds__(NT, 1) void k_cnn_act(CnnNet net, const uint16_t *wb, const uint8_t *pixels, int n, int channels, float epsilon,
                                                   uint64_t seed, uint32_t call, int32_t *actions, float *qvalues) {
    __shared__ __attribute__((aligned(16))) uint8_t STG[4][FRAME_BYTES]; // a frame per wavefront; after the convolutions: H3 and Q
    __shared__ __attribute__((aligned(16))) uint16_t H1[4][H1_IMG];
    __shared__ __attribute__((aligned(16))) uint16_t H2[TM * LDH2];
    uint16_t *H3 = reinterpret_cast<uint16_t *>(&STG[0][0]);               // [TM][LDH3] bf16
    float *Q = reinterpret_cast<float *>(&STG[0][0] + TM * LDH3 * 2);      // [TM][8]
    const int t = threadIdx.x, w = t >> 6, l = t & 63, r16 = l & 15, g = l >> 4;
    const int stack = channels / 3, k1 = channels * 64;
    const uint16_t *wc1 = wb, *wc2 = wc1 + 16 * k1, *wf1 = wc2 + W2_COUNT, *wf2 = wf1 + W3_COUNT;
    // conv1: byte offset of this lane's output position (row r16 of M tile mt) inside a channel plane
    int off1[15];
#pragma unroll
    for (int mt = 0; mt < 15; mt++) {
        const int p = min(16 * mt + r16, 224);
        off1[mt] = (4 * (p / 15)) * 64 + 4 * (p % 15);
    }
    // conv2: element offset of this lane's output position inside a channel of H1
    int off2[3];
#pragma unroll
    for (int mt = 0; mt < 3; mt++) {
        const int p = min(16 * mt + r16, 35);
        off2[mt] = (2 * (p / 6)) * 16 + 2 * (p % 6);
    }
    const int ntiles = (n + TM - 1) / TM;
    const int nitems = (TM / 4) * stack;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        uint4 pre[12];
        f4v acc1[15];
        load_frame(pre, pixels, tile * TM + w, n, channels, 0, l);
        int round = 0, f = 0;
        for (int q = 0; q < nitems; q++) {
            __syncthreads(); // the stage (and what aliases it) is free
            {
                uint4 *dst = reinterpret_cast<uint4 *>(&STG[w][0]);
#pragma unroll
                for (int i = 0; i < 12; i++) dst[i * 64 + l] = pre[i];
            }
            __syncthreads();
            {
                const int fn = f + 1 < stack ? f + 1 : 0, rn = f + 1 < stack ? round : round + 1;
                if (q + 1 < nitems) load_frame(pre, pixels, tile * TM + rn * 4 + w, n, channels, fn, l);
            }
            if (f == 0) {
#pragma unroll
                for (int mt = 0; mt < 15; mt++) acc1[mt] = (f4v)0.0f;
            }
            // ---- conv1, this frame's share of K: 3 channels x 64 = 6 steps of 32 (a step = 4 rows of the 8 x 8 window)
#pragma unroll
            for (int s = 0; s < 6; s++) {
                const uint4 b = *reinterpret_cast<const uint4 *>(wc1 + r16 * k1 + (3 * f) * 64 + 32 * s + 8 * g);
                const uint8_t *plane = &STG[w][0] + (s >> 1) * 4096 + (4 * (s & 1) + g) * 64;
#pragma unroll
                for (int mt = 0; mt < 15; mt++) {
                    const uint32_t *px = reinterpret_cast<const uint32_t *>(plane + off1[mt]);
                    uint4 a;
                    pixels4(px[0], a.x, a.y);
                    pixels4(px[1], a.z, a.w);
                    acc1[mt] = mfma(a, b, acc1[mt]);
                }
            }
            if (f == stack - 1) { // (uniform over the workgroup: the barriers below are reached by everyone)
                // ---- conv1's epilogue: column = channel r16, rows = positions 16 mt + 4 g + r
                {
                    const float bias = net.b1[r16];
#pragma unroll
                    for (int mt = 0; mt < 15; mt++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int p = 16 * mt + 4 * g + r;
                            if (p < 225) H1[w][r16 * 240 + (p / 15) * 16 + (p % 15)] = (uint16_t)bf16_rne(relu(acc1[mt][r] * 0.00390625f + bias));
                        }
                }
                __syncthreads();
                // ---- conv2: K = (ic, ky, kx) = 8 steps of 32 (a step = 2 input channels; a lane's 8 = rows ky0, ky0 + 1 of one channel)
                f4v acc2[3][2];
#pragma unroll
                for (int mt = 0; mt < 3; mt++) { acc2[mt][0] = (f4v)0.0f; acc2[mt][1] = (f4v)0.0f; }
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const uint4 b0 = *reinterpret_cast<const uint4 *>(wc2 + r16 * 256 + 32 * s + 8 * g);
                    const uint4 b1 = *reinterpret_cast<const uint4 *>(wc2 + (16 + r16) * 256 + 32 * s + 8 * g);
                    const uint16_t *chan = &H1[w][0] + (2 * s + (g >> 1)) * 240 + (2 * (g & 1)) * 16;
#pragma unroll
                    for (int mt = 0; mt < 3; mt++) {
                        const uint32_t *px = reinterpret_cast<const uint32_t *>(chan + off2[mt]);
                        const uint4 a = make_uint4(px[0], px[1], px[8], px[9]);
                        acc2[mt][0] = mfma(a, b0, acc2[mt][0]);
                        acc2[mt][1] = mfma(a, b1, acc2[mt][1]);
                    }
                }
                {
                    uint16_t *row = &H2[(round * 4 + w) * LDH2];
#pragma unroll
                    for (int nt = 0; nt < 2; nt++) {
                        const int oc = 16 * nt + r16;
                        const float bias = net.b2[oc];
#pragma unroll
                        for (int mt = 0; mt < 3; mt++) {
                            const int p0 = 16 * mt + 4 * g; // four consecutive positions: all below 36 or none
                            if (p0 < 36) {
                                const uint32_t v0 = bf16_rne(relu(acc2[mt][nt][0] + bias)), v1 = bf16_rne(relu(acc2[mt][nt][1] + bias));
                                const uint32_t v2 = bf16_rne(relu(acc2[mt][nt][2] + bias)), v3 = bf16_rne(relu(acc2[mt][nt][3] + bias));
                                *reinterpret_cast<uint2 *>(row + oc * 36 + p0) = make_uint2(v0 | (v1 << 16), v2 | (v3 << 16));
                            }
                        }
                    }
                }
            }
            if (++f == stack) { f = 0; round++; }
        }
        __syncthreads();
        // ---- fc1: [32 x 1152] x [1152 x 256]; wavefront w: outputs 64 w .. 64 w + 63 (4 N tiles) x both M tiles
        {
            f4v acc3[2][4];
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc3[mt][j] = (f4v)0.0f;
            const uint16_t *arow = &H2[r16 * LDH2 + 8 * g];
            const uint16_t *brow = wf1 + (size_t)(64 * w + r16) * FLAT + 8 * g;
#pragma unroll 4
            for (int s = 0; s < FLAT / 32; s++) {
                const uint4 a0 = *reinterpret_cast<const uint4 *>(arow + 32 * s);
                const uint4 a1 = *reinterpret_cast<const uint4 *>(arow + 16 * LDH2 + 32 * s);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint4 b = *reinterpret_cast<const uint4 *>(brow + (size_t)(16 * j) * FLAT + 32 * s);
                    acc3[0][j] = mfma(a0, b, acc3[0][j]);
                    acc3[1][j] = mfma(a1, b, acc3[1][j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int col = 64 * w + 16 * j + r16;
                const float bias = net.b3[col];
#pragma unroll
                for (int mt = 0; mt < 2; mt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) H3[(16 * mt + 4 * g + r) * LDH3 + col] = (uint16_t)bf16_rne(relu(acc3[mt][j][r] + bias));
            }
        }
        __syncthreads();
        // ---- fc2: 8 outputs in one 16-wide N tile (columns 8..15: zero weights), M tile w on wavefronts 0 and 1
        if (w < 2) {
            f4v acc4 = (f4v)0.0f;
#pragma unroll
            for (int s = 0; s < HID / 32; s++) {
                const uint4 a = *reinterpret_cast<const uint4 *>(&H3[(16 * w + r16) * LDH3 + 32 * s + 8 * g]);
                uint4 b = make_uint4(0u, 0u, 0u, 0u);
                if (r16 < NA) b = *reinterpret_cast<const uint4 *>(wf2 + r16 * HID + 32 * s + 8 * g);
                acc4 = mfma(a, b, acc4);
            }
            if (r16 < NA) {
                const float bias = net.b4[r16];
#pragma unroll
                for (int r = 0; r < 4; r++) Q[(16 * w + 4 * g + r) * NA + r16] = acc4[r] + bias;
            }
        }
        __syncthreads();
        if (t < TM) {
            const int row = tile * TM + t;
            if (row < n) {
                int best = 0;
                float mx = Q[t * NA];
#pragma unroll
                for (int a = 1; a < NA; a++) { const float qa = Q[t * NA + a]; if (qa > mx) { mx = qa; best = a; } }
                actions[row] = epsilon_greedy(best, row, call, seed, epsilon);
                if (qvalues) {
#pragma unroll
                    for (int a = 0; a < NA; a++) qvalues[(size_t)row * NA + a] = Q[t * NA + a];
                }
            }
        }
    }
}

} // namespace

extern "C" int rr_cnn_act(rr_dqn *d, const float *const params[8], const uint8_t *pixels, int32_t n, int32_t channels, float epsilon,
                          uint64_t seed, uint32_t call, int32_t *actions, float *qvalues, void *stream) {
    if (!d || !params || !pixels || !actions) return rr_dqn_fail(-1, "rr_cnn_act: null argument");
    for (int k = 0; k < 8; k++) if (!params[k]) return rr_dqn_fail(-1, "rr_cnn_act: null parameter pointer");
    if (channels != 3 && channels != 6 && channels != 9 && channels != 12) return rr_dqn_fail(-1, "rr_cnn_act: channels must be 3, 6, 9 or 12");
    if (n < 1 || n > (1 << 22)) return rr_dqn_fail(-1, "rr_cnn_act: the number of rows must be in 1 .. 1<<22");
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return rr_dqn_fail(-1, "rr_cnn_act: epsilon must be in [0, 1]");
    if ((uintptr_t)pixels % 16) return rr_dqn_fail(-1, "rr_cnn_act: pixels must be 16-byte aligned");
    int prev = -1;
    const bool sw = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
    if (!d->cnn_weights && hipMalloc((void **)&d->cnn_weights, sizeof(uint16_t) * SCRATCH_ELEMS) != hipSuccess) {
        d->cnn_weights = nullptr;
        if (sw) (void)hipSetDevice(prev);
        return rr_dqn_fail(-3, "rr_cnn_act: out of device memory");
    }
    CnnNet net = { params[0], params[1], params[2], params[3], params[4], params[5], params[6], params[7] };
    const int w1_count = 16 * channels * 64;
    hipLaunchKernelGGL(k_cnn_prep, dim3(256), dim3(256), 0, (hipStream_t)stream, net, w1_count, d->cnn_weights);
    const int ntiles = (n + TM - 1) / TM, nwg = ntiles < d->nwg ? ntiles : d->nwg;
    hipLaunchKernelGGL(k_cnn_act, dim3(nwg), dim3(NT), 0, (hipStream_t)stream, net, (const uint16_t *)d->cnn_weights, pixels, (int)n, (int)channels,
                       epsilon, seed, call, actions, qvalues);
    const hipError_t e = hipGetLastError();
    if (sw) (void)hipSetDevice(prev);
    if (e != hipSuccess) return rr_dqn_fail(-2, hipGetErrorString(e));
    return 0;
}
