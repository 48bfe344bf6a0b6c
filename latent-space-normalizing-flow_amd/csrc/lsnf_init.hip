// lsnf_init.hip -- data-dependent actnorm initialisation (Glow's init; reference model.py:235-262 with init=True,
// threaded through revnet2d_step.forward :389-422 and fc.forward :324-331).
//
// For block k = 0 .. depth-1, on x = the block's input (z for k = 0, else block k-1's output under its NEW parameters):
//   actnorm      : b := -mean_b x;  logs := log(1 / (sqrt(mean_b (x+b)^2) + 1e-6)) / 3            (params 0, 1)
//   y = actnorm(x) @ W;  u1 = y[:, :nz/2] @ fc_1.w          -> fc_1.actnorm from u1 the same way    (params 4, 5)
//   u2 = relu(actnorm(u1)) @ fc_2.w                         -> fc_2.actnorm from u2                 (params 7, 8)
//   hf = (relu(actnorm(u2)) @ fc_zeros.w + b) * exp(3 logs), then the coupling -> the next block's input
// Per stage, launches on the caller's stream:
//   lsnf_init_gemm     : one GEMM of the chain, fp32 FMA; the weight matrix stays in LDS while the workgroup walks its
//                        32-row tiles; prologue = the actnorm (+ relu) of the input, epilogue = plain store or the coupling
//                        (written in place over the second half of y, which then is the block's output).
//   lsnf_init_colstats : per 64-row chunk, the fp64 column sums of x and x^2 in a fixed order -> one slab per chunk.
//   lsnf_init_finalize : one workgroup per column folds the slabs in a fixed order (strided partials + LDS tree) and writes
//                        b and logs.  No atomics anywhere: the result is bit-for-bit the same on every run, whatever the grid.
// mean_b (x+b)^2 with b the stored fp32 value is E[x^2] + 2 b E[x] + b^2 in fp64 (one pass over the data).
// Workspace (bytes): [slabs: nslab x 128 x 2 doubles][y: 2 x B x nz floats (ping-pong)][u1: B x width][u2: B x width].
#include <hip/hip_runtime.h>
#include "../../include/lsnf_flow.h"
#include "lsnf_layout.h"
#include "lsnf_launch.h"

namespace {

enum { P_AB = 0, P_ALOGS, P_W, P_W1, P_B1, P_LOGS1, P_W2, P_B2, P_LOGS2, P_W3, P_B3, P_LOGS3 };

constexpr int kStatRows = 64;    // rows per slab of column sums
constexpr int kTileRows = 32;    // rows per GEMM tile
constexpr int kMaxGemmGrid = 1024;

size_t slab_count(int B) { return ((size_t)B + kStatRows - 1) / kStatRows; }
size_t slab_bytes(int B) { return slab_count(B) * 128 * 2 * sizeof(double); }

__global__ __launch_bounds__(256) void lsnf_init_colstats(const float* __restrict__ x, int B, int N, double* __restrict__ slab) {
    __shared__ double ps[128], pq[128];
    const int t = threadIdx.x, n = t & 127, rg = t >> 7;
    const int r0 = blockIdx.x * kStatRows, r1 = min(B, r0 + kStatRows);
    double s = 0.0, q = 0.0;
    if (n < N)
        for (int r = r0 + rg; r < r1; r += 2) {
            const double v = x[(size_t)r * N + n];
            s += v;
            q += v * v;
        }
    if (rg == 1) { ps[n] = s; pq[n] = q; }
    __syncthreads();
    if (rg == 0 && n < N) {
        double* o = slab + ((size_t)blockIdx.x * 128 + n) * 2;
        o[0] = s + ps[n];
        o[1] = q + pq[n];
    }
}

__global__ __launch_bounds__(256) void lsnf_init_finalize(const double* __restrict__ slab, int nslab, int B,
                                                          float* __restrict__ b_out, float* __restrict__ logs_out) {
    __shared__ double rs[256], rq[256];
    const int n = blockIdx.x, t = threadIdx.x;
    double s = 0.0, q = 0.0;
    for (int g = t; g < nslab; g += 256) {
        s += slab[((size_t)g * 128 + n) * 2];
        q += slab[((size_t)g * 128 + n) * 2 + 1];
    }
    rs[t] = s;
    rq[t] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { rs[t] += rs[t + w]; rq[t] += rq[t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        const double mean = rs[0] / B;
        const float bf = (float)(-mean);                               // model.py:238-241
        const double bd = bf;
        const double var = fmax(rq[0] / B + 2.0 * bd * mean + bd * bd, 0.0);   // mean of (x + b)^2, model.py:253
        b_out[n] = bf;
        logs_out[n] = (float)(log(1.0 / (sqrt(var) + 1e-6)) / 3.0);   // model.py:260-262, scale 1, logscale_factor 3
    }
}

// PRO: 0 = none, 1 = actnorm (x + b) * exp(3 logs), 2 = actnorm + relu.   EPI: 0 = store, 1 = affine coupling, 2 = additive.
// CP threads per row group (64 or 128 >= N), 256 / CP row groups, each thread kTileRows * CP / 256 rows of one column.
template <int CP, int PRO, int EPI>
__global__ __launch_bounds__(256) void lsnf_init_gemm(const float* __restrict__ in, int ld_in, int K, const float* __restrict__ W,
                                                      int N, const float* __restrict__ pb, const float* __restrict__ plogs,
                                                      float* __restrict__ out, const float* __restrict__ fzb,
                                                      const float* __restrict__ fzlogs, int half, int B) {
    constexpr int RG = 256 / CP, RPT = kTileRows / RG;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int KP = (K + 3) & ~3;
    float* Ws = smem;                       // KP x N, rows >= K zero
    float* As = Ws + KP * N;                // kTileRows x KP, prologue applied, padding zero
    float* Hs = As + kTileRows * KP;        // kTileRows x N (coupling epilogue)
    const int t = threadIdx.x, n = t % CP, rg = t / CP;
    const int nn = n < N ? n : N - 1;       // idle columns read valid LDS, their results are dropped

    for (int i = t; i < KP * N; i += 256) {
        const int k = i / N;
        Ws[i] = k < K ? W[i] : 0.0f;
    }
    const int ntiles = (B + kTileRows - 1) / kTileRows;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int row0 = tile * kTileRows;
        __syncthreads();
        for (int i = t; i < kTileRows * KP; i += 256) {
            const int r = i / KP, k = i % KP, row = row0 + r;
            float v = 0.0f;
            if (row < B && k < K) {
                v = in[(size_t)row * ld_in + k];
                if (PRO) {     // model.py:244,264-268 (from global: a static LDS array would cost the 128x128 GEMM its
                               // second workgroup per CU -- 64 KiB of weights + 16 KiB of tile is exactly half the LDS)
                    v = (v + pb[k]) * expf(plogs[k] * 3.0f);
                    if (PRO == 2) v = fmaxf(v, 0.0f);
                }
            }
            As[i] = v;
        }
        __syncthreads();
        float acc[RPT];
#pragma unroll
        for (int i = 0; i < RPT; ++i) acc[i] = 0.0f;
        for (int k = 0; k < KP; k += 4) {
            const float w0 = Ws[(k + 0) * N + nn], w1 = Ws[(k + 1) * N + nn];
            const float w2 = Ws[(k + 2) * N + nn], w3 = Ws[(k + 3) * N + nn];
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const float4 a = *reinterpret_cast<const float4*>(As + (rg + RG * i) * KP + k);
                acc[i] = fmaf(a.x, w0, acc[i]);
                acc[i] = fmaf(a.y, w1, acc[i]);
                acc[i] = fmaf(a.z, w2, acc[i]);
                acc[i] = fmaf(a.w, w3, acc[i]);
            }
        }
        if (EPI == 0) {
            if (n < N) {
#pragma unroll
                for (int i = 0; i < RPT; ++i) {
                    const int row = row0 + rg + RG * i;
                    if (row < B) out[(size_t)row * N + n] = acc[i];
                }
            }
        } else {
            if (n < N) {
                const float fb = fzb[n], fs = expf(fzlogs[n] * 3.0f);               // model.py:347-349
#pragma unroll
                for (int i = 0; i < RPT; ++i) Hs[(rg + RG * i) * N + n] = (acc[i] + fb) * fs;
            }
            __syncthreads();
            const int nz = 2 * half;
            for (int i = t; i < kTileRows * half; i += 256) {
                const int r = i / half, j = i % half, row = row0 + r;
                if (row >= B) continue;
                float* yp = out + (size_t)row * nz + half + j;
                if (EPI == 1) {                                                     // model.py:410-415
                    const float shift = Hs[r * N + 2 * j];
                    const float scale = 1.0f / (1.0f + expf(-(Hs[r * N + 2 * j + 1] + 2.0f)));
                    *yp = (*yp + shift) * scale;
                } else {                                                            // model.py:407-408
                    *yp = *yp + Hs[r * N + j];
                }
            }
        }
    }
}

template <int PRO, int EPI>
hipError_t launch_gemm(int B, const float* in, int ld_in, int K, const float* W, int N, const float* pb, const float* plogs,
                       float* out, const float* fzb, const float* fzlogs, int half, hipStream_t stream) {
    const int KP = (K + 3) & ~3;
    const size_t lds = sizeof(float) * ((size_t)KP * N + (size_t)kTileRows * KP + (EPI ? (size_t)kTileRows * N : 0));
    const int ntiles = (B + kTileRows - 1) / kTileRows;
    const int grid = ntiles < kMaxGemmGrid ? ntiles : kMaxGemmGrid;
    auto kern = N <= 64 ? lsnf_init_gemm<64, PRO, EPI> : lsnf_init_gemm<128, PRO, EPI>;
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, in, ld_in, K, W, N, pb, plogs, out, fzb, fzlogs, half, B);
    return hipGetLastError();
}

hipError_t fit_actnorm(const float* x, int B, int N, double* slab, float* b_out, float* logs_out, hipStream_t stream) {
    const int nslab = (int)slab_count(B);
    hipLaunchKernelGGL(lsnf_init_colstats, dim3(nslab), dim3(256), 0, stream, x, B, N, slab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lsnf_init_finalize, dim3(N), dim3(256), 0, stream, slab, nslab, B, b_out, logs_out);
    return hipGetLastError();
}

}  // namespace

size_t lsnf_init_workspace_bytes(const LsnfGeo& g, int B) {
    return slab_bytes(B) + sizeof(float) * ((size_t)B * (2 * (size_t)g.nz + 2 * (size_t)g.width));
}

hipError_t lsnf_launch_actnorm_init(const LsnfInitCall& c) {
    const LsnfGeo& g = c.g;
    float* const* params_host = c.params_host;
    const int B = c.B;
    const float* z_in = c.z_in;
    void* workspace = c.workspace;
    const hipStream_t stream = c.stream;
    const int nz = g.nz, half = g.half, width = g.width;
    const int n_out = g.coupling == 1 ? nz : half;
    double* slab = (double*)workspace;
    float* ybuf[2];
    ybuf[0] = (float*)((char*)workspace + slab_bytes(B));
    ybuf[1] = ybuf[0] + (size_t)B * nz;
    float* u1 = ybuf[1] + (size_t)B * nz;
    float* u2 = u1 + (size_t)B * width;
    const float* x = z_in;
    hipError_t e = hipSuccess;
#define LSNF_TRY(call) do { e = (call); if (e != hipSuccess) return e; } while (0)
    for (int k = 0; k < g.depth; ++k) {
        float* const* P = params_host + (size_t)k * LSNF_PARAMS_PER_BLOCK;
        float* y = ybuf[k & 1];
        LSNF_TRY(fit_actnorm(x, B, nz, slab, P[P_AB], P[P_ALOGS], stream));                                  // model.py:392
        LSNF_TRY((launch_gemm<1, 0>(B, x, nz, nz, P[P_W], nz, P[P_AB], P[P_ALOGS], y, nullptr, nullptr, half, stream)));
        LSNF_TRY((launch_gemm<0, 0>(B, y, nz, half, P[P_W1], width, nullptr, nullptr, u1, nullptr, nullptr, half, stream)));
        LSNF_TRY(fit_actnorm(u1, B, width, slab, P[P_B1], P[P_LOGS1], stream));                             // model.py:307,328
        LSNF_TRY((launch_gemm<2, 0>(B, u1, width, width, P[P_W2], width, P[P_B1], P[P_LOGS1], u2, nullptr, nullptr, half,
                                    stream)));
        LSNF_TRY(fit_actnorm(u2, B, width, slab, P[P_B2], P[P_LOGS2], stream));                             // model.py:308,328
        if (k + 1 < g.depth) {      // the last block's output feeds no statistic
            if (g.coupling == 1)
                LSNF_TRY((launch_gemm<2, 1>(B, u2, width, width, P[P_W3], n_out, P[P_B2], P[P_LOGS2], y, P[P_B3], P[P_LOGS3],
                                            half, stream)));
            else
                LSNF_TRY((launch_gemm<2, 2>(B, u2, width, width, P[P_W3], n_out, P[P_B2], P[P_LOGS2], y, P[P_B3], P[P_LOGS3],
                                            half, stream)));
        }
        x = y;
    }
#undef LSNF_TRY
    return e;
}
