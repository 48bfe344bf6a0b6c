// lsnf_optim.hip -- the flow's optimizer step on the device: global-norm clip (torch's clip_grad_norm_) + Adam (torch's
// _single_tensor_adam; with flags: amsgrad, maximize, AdamW's decoupled decay, a skip of the whole step on a non-finite norm
// and an exponential moving average of the written parameters) over the depth x 12 live tensors; reference
// train.py:413-415 (`clip_grad_norm_`, `optF.step()`).  At most two stream-ordered launches, no atomics, no grid-wide barrier:
//
//   lsnf_grad_norm_kernel (only with clipping or a norm output): float64 partial sums of g^2, one per workgroup, into the
//                        state header.  Fixed assignment of elements to workgroups and a fixed order inside each.
//   lsnf_adam_kernel    : every workgroup folds the partials in the same fixed order (float64), derives the clip coefficient and
//                        the bias corrections once (float64, broadcast through LDS) and updates its elements: float64 math on
//                        the stored fp32 values, one rounding per stored value.
//
// Work units.  Every tensor is cut into chunks of kChunk = 1024 consecutive elements (the last one short); the chunks of the
// call are numbered block by block, tensor by tensor, and workgroup w of a grid of G = min(chunks, LSNF_ADAM_MAX_GROUPS)
// takes chunks w, w + G, w + 2G, ...  Thread t of the workgroup owns elements 4t .. 4t+3 of a chunk -- as one 16-byte access
// where the tensor's pointers allow it, as four 4-byte accesses otherwise; the assignment, the order of every sum and the
// element math are the same either way, so the choice cannot change a bit of the result.
//
// Step counter.  One launch cannot both read and advance a shared counter without a grid-wide barrier (a workgroup that
// starts late would read the advanced value), so every workgroup keeps ITS OWN int64 counter in the header: workgroup w reads
// counter[w], uses counter[w] + 1 as `step` and stores it back.  Every call runs the same G workgroups (G follows from the
// geometry alone), so all counters agree at all times and counter[0] -- byte 0 of the state -- is the step count.  The same
// scheme with and without the norm launch; the norm kernel never touches the counters.
//
// Variants.  AMSGRAD and EMA add an array behind v in the state (vmax, then the average) and its loads and stores: template
// flags, so the plain step carries none of it.  DECOUPLED is one as well (as a run-time branch it cost the plain step 10
// VGPRs).  MAXIMIZE is the sign of the clip coefficient and SKIP_NONFINITE a workgroup-uniform branch on the flags word.
// Skip: every workgroup folds the same partials in the same order, so all reach the same verdict on the norm, and a
// non-finite one makes every workgroup leave before it has written anything but (workgroup 0) the norm and the skipped count.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/lsnf_flow.h"
#include "lsnf_layout.h"
#include "lsnf_launch.h"

namespace {

constexpr int kChunk = 1024;         // elements per chunk = 256 threads x 4
constexpr int kThreads = 256;

struct LsnfAdamPtrs { float* p[LSNF_MAX_DEPTH * 12]; };
struct LsnfAdamGradPtrs { const float* p[LSNF_MAX_DEPTH * 12]; };

struct AdamGeo {
    int size[12];                    // elements of the 12 tensors of one block, ABI order
    int depth;
    int chunks_per_block;            // sum_j ceil(size[j] / kChunk)
    int per_block;                   // sum_j size[j]
    int nchunks;                     // depth * chunks_per_block
    long long moment_floats;         // depth * per_block rounded up to 4: floats of m (and of v)
};

struct NormArgs {
    LsnfAdamGradPtrs g;
    AdamGeo geo;
    double* partials;
};
struct AdamArgs {
    LsnfAdamPtrs p;
    LsnfAdamGradPtrs g;
    AdamGeo geo;
    char* state;
    const float* lr_dev;
    float* norm_out;
    double lr, beta1, beta2, eps, weight_decay, max_norm, ema_decay;
    int nparts;                      // partials the norm launch wrote (0: no norm launch)
    unsigned flags;                  // LSNF_ADAM_MAXIMIZE | _SKIP_NONFINITE (AMSGRAD, EMA and DECOUPLED select the kernel)
};
static_assert(sizeof(AdamArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// chunk c -> tensor (index into the pointer tables), first element inside the tensor, the tensor's size and its element
// offset inside m / v.  Workgroup-uniform: scalar work.
struct ChunkAt { int tensor, first, size; long long moment_off; };
__device__ __forceinline__ ChunkAt locate(const AdamGeo& geo, int c) {
    const int blk = c / geo.chunks_per_block;
    int r = c - blk * geo.chunks_per_block, j = 0, pre = 0;
    for (; j < 11; ++j) {
        const int n = (geo.size[j] + kChunk - 1) / kChunk;
        if (r < n) break;
        r -= n;
        pre += geo.size[j];
    }
    return {blk * 12 + j, r * kChunk, geo.size[j], (long long)blk * geo.per_block + pre};
}
__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// elements e .. e+3 (those below n) of a tensor; `vec`: the pointer is 16-byte aligned (and e is a multiple of 4)
__device__ __forceinline__ void load4(const float* __restrict__ base, int e, int n, bool vec, float (&x)[4]) {
    if (vec && e + 3 < n) {
        const float4 q = *reinterpret_cast<const float4*>(base + e);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = e + k < n ? base[e + k] : 0.0f;
    }
}
__device__ __forceinline__ void store4(float* __restrict__ base, int e, int n, bool vec, const float (&x)[4]) {
    if (vec && e + 3 < n) {
        *reinterpret_cast<float4*>(base + e) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < n) base[e + k] = x[k];
    }
}

__global__ __launch_bounds__(kThreads) void lsnf_grad_norm_kernel(NormArgs a) {
    __shared__ double red[kThreads];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int c = blockIdx.x; c < a.geo.nchunks; c += gridDim.x) {
        const ChunkAt at = locate(a.geo, c);
        const float* g = a.g.p[at.tensor];
        if (!g) continue;                                   // grad is None: contributes 0
        float x[4];
        load4(g, at.first + 4 * t, at.size, al16(g), x);    // (elements past the tensor's end read as 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)x[k] * (double)x[k];
    }
    red[t] = acc;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) a.partials[blockIdx.x] = red[0];
}

template <bool AMSGRAD, bool EMA, bool DECOUPLED>
__global__ __launch_bounds__(kThreads) void lsnf_adam_kernel(AdamArgs a) {
    __shared__ double parts[LSNF_ADAM_MAX_GROUPS], lane_sum[16];
    __shared__ double sc[3];                                // coef, -lr / bc1, sqrt(bc2)
    const int t = threadIdx.x;
    float* const mom = reinterpret_cast<float*>(a.state + LSNF_ADAM_HEADER_BYTES);
    const bool clip = a.max_norm > 0.0;
    // MAXIMIZE is the sign of the clip coefficient: (-c) * g == -(c * g) bit for bit, and -1 * g is the exact negation
    const bool maximize = (a.flags & LSNF_ADAM_MAXIMIZE) != 0;
    const bool scale = clip || maximize;
    const double b1 = a.beta1, w1 = 1.0 - a.beta1, b2 = a.beta2, w2 = 1.0 - a.beta2, eps = a.eps, wd = a.weight_decay;
    bool first = true;
    double coef = 1.0, neg_step = 0.0, bc2_sqrt = 1.0;
    for (int c = blockIdx.x; c < a.geo.nchunks; c += gridDim.x) {
        const ChunkAt at = locate(a.geo, c);
        float* p = a.p.p[at.tensor];
        const float* g = a.g.p[at.tensor];
        float* m = mom + at.moment_off;
        float* v = m + a.geo.moment_floats;
        float* vmax = v + a.geo.moment_floats;                                 // (AMSGRAD only)
        float* ema = v + (AMSGRAD ? 2 : 1) * a.geo.moment_floats;              // (EMA only)
        const bool live = g != nullptr;                     // grad is None: parameter, m, v and vmax keep their bits
        const bool vec = al16(p) && al16(g) && al16(m) && al16(v);            // (vmax and the average sit as m does: N % 4 == 0)
        const int e = at.first + 4 * t, n = at.size;
        float xp[4], xg[4], xm[4], xv[4], xx[4], xe[4];
        if (live || EMA) load4(p, e, n, vec, xp);           // the loads are in flight while the scalars are derived
        if (live) {
            load4(g, e, n, vec, xg);
            load4(m, e, n, vec, xm);
            load4(v, e, n, vec, xv);
            if (AMSGRAD) load4(vmax, e, n, vec, xx);
        }
        if (EMA) load4(ema, e, n, vec, xe);
        if (first) {
            first = false;
            // every load of the prologue is issued at once (the partials by all threads, the counter and the device lr by
            // thread 0); then the partials in a fixed order: lane l of the first 16 sums partials 16 l .. 16 l + 15 in index
            // order, thread 0 sums the 16 lane sums in index order
            long long* const counter = reinterpret_cast<long long*>(a.state + LSNF_ADAM_STEP_OFFSET) + blockIdx.x;
            long long step0 = 0;
            float lr_loaded = 0.0f;
            parts[t] = t < a.nparts ? reinterpret_cast<const double*>(a.state + LSNF_ADAM_PARTIALS_OFFSET)[t] : 0.0;
            if (t == 0) {
                step0 = *counter;
                if (a.lr_dev) lr_loaded = *a.lr_dev;
            }
            __syncthreads();
            if (t < 16) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) s += parts[16 * t + i];
                lane_sum[t] = s;
            }
            __syncthreads();
            if (t == 0) {
                const long long step = step0 + 1;
                double cf = 1.0;
                bool skip = false;
                if (a.nparts > 0) {
                    double ss = 0.0;
                    for (int i = 0; i < 16; ++i) ss += lane_sum[i];
                    const double norm = sqrt(ss);
                    if (clip) {
                        const double r = a.max_norm / (norm + 1e-6);      // clip_grad_norm_; a NaN norm gives a NaN coefficient
                        cf = r > 1.0 ? 1.0 : r;
                    }
                    skip = (a.flags & LSNF_ADAM_SKIP_NONFINITE) != 0 && !isfinite(norm);
                    if (blockIdx.x == 0) {
                        *reinterpret_cast<float*>(a.state + LSNF_ADAM_NORM_OFFSET) = (float)norm;
                        if (a.norm_out) *a.norm_out = (float)norm;
                        if (skip) {                                       // one writer, a plain load and store
                            long long* const skipped = reinterpret_cast<long long*>(a.state + LSNF_ADAM_SKIPPED_OFFSET);
                            *skipped = *skipped + 1;
                        }
                    }
                }
                if (!skip) *counter = step;
                const double lr = a.lr_dev ? (double)lr_loaded : a.lr;
                const double bc1 = 1.0 - pow(a.beta1, (double)step), bc2 = 1.0 - pow(a.beta2, (double)step);
                sc[0] = maximize ? -cf : cf;
                sc[1] = -(lr / bc1);
                sc[2] = sqrt(bc2);
                // the partials have been consumed (second barrier above): their first slots carry the variants' scalars
                parts[0] = __dsub_rn(1.0, __dmul_rn(lr, wd));             // AdamW's 1 - lr * weight_decay
                parts[1] = skip ? 1.0 : 0.0;
                parts[2] = step == 1 ? 1.0 : 0.0;
            }
            __syncthreads();
            coef = sc[0]; neg_step = sc[1]; bc2_sqrt = sc[2];
        }
        if ((a.flags & LSNF_ADAM_SKIP_NONFINITE) != 0 && parts[1] != 0.0) return;      // the same verdict in every workgroup
        if (!live && !EMA) continue;
        // Element math in float64 from the stored fp32 values, ONE rounding per stored value: p, m and v are the correctly
        // rounded results of the formulas (fp32 arithmetic would add two to four roundings and the fp32 images of 1 - beta:
        // up to 1.4 ulp on v after a single step).  Explicit intrinsics: contraction choices do not decide the bits.
        const double w_ema = 1.0 - a.ema_decay;
        const bool ema_starts = EMA && parts[2] != 0.0;     // step 1: the average starts from the parameters as this step finds them
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double p_old = xp[k];
            if (live) {
                double gk = xg[k];
                double pk = p_old;
                if (scale) gk = __dmul_rn(coef, gk);                              // a coefficient of exactly 1 leaves the bits
                if (wd != 0.0) {
                    if (DECOUPLED) pk = __dmul_rn(pk, parts[0]);
                    else gk = __fma_rn(wd, pk, gk);
                }
                const double mk = __fma_rn(w1, gk, __dmul_rn(b1, (double)xm[k]));   // = m + (1 - beta1) (g - m)
                const double vk = __fma_rn(__dmul_rn(w2, gk), gk, __dmul_rn(b2, (double)xv[k]));
                double root = vk;
                if (AMSGRAD) {
                    root = fmax((double)xx[k], vk);                               // the max takes the unrounded v
                    xx[k] = (float)root;
                }
                const double den = __dadd_rn(__ddiv_rn(__dsqrt_rn(root), bc2_sqrt), eps);
                xp[k] = (float)__fma_rn(neg_step, __ddiv_rn(mk, den), pk);
                xm[k] = (float)mk;
                xv[k] = (float)vk;
            }
            if (EMA) {                                      // of the STORED parameter; a tensor without a gradient takes part
                const double e_prev = ema_starts ? p_old : (double)xe[k];
                xe[k] = (float)__fma_rn(w_ema, __dsub_rn((double)xp[k], e_prev), e_prev);
            }
        }
        if (live) {
            store4(p, e, n, vec, xp);
            store4(m, e, n, vec, xm);
            store4(v, e, n, vec, xv);
            if (AMSGRAD) store4(vmax, e, n, vec, xx);
        }
        if (EMA) store4(ema, e, n, vec, xe);
    }
}

void adam_geo(AdamGeo* a, const LsnfGeo& g) {
    const int nz = g.nz, half = g.half, w = g.width, n_out = g.coupling == 1 ? nz : half;
    const int size[12] = {nz, nz, nz * nz, half * w, w, w, w * w, w, w, w * n_out, n_out, n_out};
    a->depth = g.depth;
    a->chunks_per_block = 0;
    a->per_block = 0;
    for (int j = 0; j < 12; ++j) {
        a->size[j] = size[j];
        a->chunks_per_block += (size[j] + kChunk - 1) / kChunk;
        a->per_block += size[j];
    }
    a->nchunks = g.depth * a->chunks_per_block;
    a->moment_floats = ((long long)g.depth * a->per_block + 3) & ~3ll;
}

}  // namespace

size_t lsnf_adam_bytes(const LsnfGeo& g, unsigned flags) {
    AdamGeo a;
    adam_geo(&a, g);
    const int arrays = 2 + ((flags & LSNF_ADAM_AMSGRAD) ? 1 : 0) + ((flags & LSNF_ADAM_EMA) ? 1 : 0);      // m, v, vmax, average
    return (size_t)LSNF_ADAM_HEADER_BYTES + arrays * sizeof(float) * (size_t)a.moment_floats;
}

hipError_t lsnf_launch_adam(const LsnfAdamCall& c) {
    AdamGeo geo;
    adam_geo(&geo, c.g);
    const int grid = geo.nchunks < LSNF_ADAM_MAX_GROUPS ? geo.nchunks : LSNF_ADAM_MAX_GROUPS;
    const int n = c.g.depth * 12;
    const bool want_norm = c.max_norm > 0.0 || c.grad_norm_out != nullptr || (c.flags & LSNF_ADAM_SKIP_NONFINITE);
    if (want_norm) {
        NormArgs na;
        for (int i = 0; i < LSNF_MAX_DEPTH * 12; ++i) na.g.p[i] = i < n ? c.grads_host[i] : nullptr;
        na.geo = geo;
        na.partials = reinterpret_cast<double*>((char*)c.state + LSNF_ADAM_PARTIALS_OFFSET);
        hipLaunchKernelGGL(lsnf_grad_norm_kernel, dim3(grid), dim3(kThreads), 0, c.stream, na);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    AdamArgs a;
    for (int i = 0; i < LSNF_MAX_DEPTH * 12; ++i) {
        a.p.p[i] = i < n ? c.params_host[i] : nullptr;
        a.g.p[i] = i < n ? c.grads_host[i] : nullptr;
    }
    a.geo = geo;
    a.state = (char*)c.state;
    a.lr_dev = c.lr_dev;
    a.norm_out = c.grad_norm_out;
    a.lr = c.lr; a.beta1 = c.beta1; a.beta2 = c.beta2; a.eps = c.eps; a.weight_decay = c.weight_decay; a.max_norm = c.max_norm;
    a.ema_decay = c.ema_decay;
    a.nparts = want_norm ? grid : 0;
    a.flags = c.flags & (LSNF_ADAM_MAXIMIZE | LSNF_ADAM_SKIP_NONFINITE);
    void (*const kernels[8])(AdamArgs) = {                  // indexed by AMSGRAD | EMA << 1 | DECOUPLED << 2
        lsnf_adam_kernel<false, false, false>, lsnf_adam_kernel<true, false, false>, lsnf_adam_kernel<false, true, false>,
        lsnf_adam_kernel<true, true, false>,   lsnf_adam_kernel<false, false, true>, lsnf_adam_kernel<true, false, true>,
        lsnf_adam_kernel<false, true, true>,   lsnf_adam_kernel<true, true, true>};
    const int which = ((c.flags & LSNF_ADAM_AMSGRAD) ? 1 : 0) | ((c.flags & LSNF_ADAM_EMA) ? 2 : 0) | ((c.flags & LSNF_ADAM_DECOUPLED) ? 4 : 0);
    hipLaunchKernelGGL(kernels[which], dim3(grid), dim3(kThreads), 0, c.stream, a);
    return hipGetLastError();
}
