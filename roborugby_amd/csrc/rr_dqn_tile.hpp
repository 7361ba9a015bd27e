// rr_dqn_tile.hpp -- the two 256-wide hidden layers of the reference's MLPs (Linear K -> 256 -> 256, ReLU; K = 11, or 11 + A for the SAC
// critics) for one 64-row tile on the fp32 matrix cores, as the kernels behind the rr_dqn handle share them: rr_dqn.hip (k_dqn_fwd_bwd,
// k_dqn_act: the Q network) and rr_sac.hip (k_sac_act: the SAC actor; k_sac_targets: actor, critics and target value net; k_sac_grads:
// the value net and the critics, forward and backward).  Device code only; what a tile's head does with X1 is the including kernel's
// business.
#pragma once
#include <hip/hip_runtime.h>

namespace rr_tile {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int H = 256, IN = 11;
constexpr int TM = 64;        // samples per tile
constexpr int LDX = TM + 1;   // LDS row stride of the transposed activations (words)
constexpr int NT = 256;       // threads per workgroup: 4 wavefronts, one per SIMD

__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// row of a 32 x 32 accumulator tile held in register r of a lane in half `half` (lanes 32-63: half = 1); its column is lane & 31
__device__ __forceinline__ int acc_row(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }

// hidden layers of one net (its members w1 [256, K], b1, w2, b2: torch.nn.Linear layouts) for the tile in Sb ([K padded to even][LDX],
// the pad row = 0; K = 11: [12][LDX], row 11 = 0): X0 = relu(fc1), X1 = relu(fc2), both transposed [feature][sample].  Every thread of the
// workgroup calls it (w = wavefront, half = lane >> 5, c = lane & 31); it ends behind a barrier: X1 is complete for every thread.
template <int K = IN, class NetT>
__device__ __forceinline__ void hidden_tile(const NetT &net, const float *Sb, float *X0, float *X1, int w, int half, int c) {
    f16v acc[4];
    // ---- fc1: K inputs (11 padded to 12), output tiles: n-tiles {2w, 2w+1} x m-tiles {0, 1}
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = (f16v)0.0f;
#pragma unroll
    for (int p = 0; p < (K + 1) / 2; p++) {
        const int k = 2 * p + half;
        const float a0 = Sb[k * LDX + c], a1 = Sb[k * LDX + 32 + c];
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            const int n = (2 * w + nt) * 32 + c;
            const float b = k < K ? net.w1[n * K + k] : 0.0f;
            acc[nt * 2 + 0] = mfma(a0, b, acc[nt * 2 + 0]);
            acc[nt * 2 + 1] = mfma(a1, b, acc[nt * 2 + 1]);
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
        const int n = (2 * w + nt) * 32 + c;
        const float bias = net.b1[n];
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float v = acc[nt * 2 + mt][r] + bias;
                X0[n * LDX + mt * 32 + acc_row(r, half)] = v > 0.0f ? v : 0.0f;
            }
    }
    __syncthreads();
    // ---- fc2: K = 256, eight k per round: a lane's float4 of W2 covers k = 8 kg + 4 half .. + 3 (the two halves of the
    // wavefront are the two k slots of an MFMA; which k a slot holds is free as long as A and B agree)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = (f16v)0.0f;
    float4 bw[2], bw_next[2];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) bw[nt] = *reinterpret_cast<const float4 *>(&net.w2[((2 * w + nt) * 32 + c) * H + 4 * half]);
#pragma unroll 2
    for (int kg = 0; kg < H / 8; kg++) {
        const int kb = kg * 8 + 4 * half;
        if (kg + 1 < H / 8) {
#pragma unroll
            for (int nt = 0; nt < 2; nt++) bw_next[nt] = *reinterpret_cast<const float4 *>(&net.w2[((2 * w + nt) * 32 + c) * H + kb + 8]);
        }
        const float bv[2][4] = { { bw[0].x, bw[0].y, bw[0].z, bw[0].w }, { bw[1].x, bw[1].y, bw[1].z, bw[1].w } };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float a0 = X0[(kb + j) * LDX + c], a1 = X0[(kb + j) * LDX + 32 + c];
#pragma unroll
            for (int nt = 0; nt < 2; nt++) {
                acc[nt * 2 + 0] = mfma(a0, bv[nt][j], acc[nt * 2 + 0]);
                acc[nt * 2 + 1] = mfma(a1, bv[nt][j], acc[nt * 2 + 1]);
            }
        }
        bw[0] = bw_next[0]; bw[1] = bw_next[1];
    }
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
        const int n = (2 * w + nt) * 32 + c;
        const float bias = net.b2[n];
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float v = acc[nt * 2 + mt][r] + bias;
                X1[n * LDX + mt * 32 + acc_row(r, half)] = v > 0.0f ? v : 0.0f;
            }
    }
    __syncthreads();
}

} // namespace rr_tile
