// ocml_ulp.hip -- the error of the device's expf and logf in units in the last place, over the argument ranges of the resampling
// move's tests (tests/hmc_resample_restated.py EXP_ULP / LOG_ULP): expf on [-140, 0], logf on [2^-5, 1].  Every argument is an fp32
// number on a fine grid; the reference is the host's double-precision function of the same fp32 argument.
//   hipcc -O3 --offload-arch=gfx950 tools/micro/ocml_ulp.hip -o tools/micro/ocml_ulp && tools/micro/ocml_ulp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void eval(const float* x, float* ex, float* lg, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { ex[i] = expf(x[i]); lg[i] = logf(x[n + i]); }
}

static double ulps(float got, double ref) {
    if (ref == 0.0) return std::fabs((double)got) / std::ldexp(1.0, -149);
    int e;
    std::frexp(ref, &e);                                      // ref = m 2^e, m in [0.5, 1): one ulp of an fp32 number there is 2^(e - 24)
    const int ue = (e - 24 < -149) ? -149 : e - 24;
    return std::fabs((double)got - ref) / std::ldexp(1.0, ue);
}

int main() {
    const int n = 1 << 22;
    std::vector<float> x(2 * n), ex(n), lg(n);
    for (int i = 0; i < n; ++i) {
        x[i] = -140.0f * (float)i / (float)(n - 1);
        x[n + i] = 0.03125f + (1.0f - 0.03125f) * (float)i / (float)(n - 1);
    }
    float *dx, *de, *dl;
    if (hipMalloc(&dx, 2 * n * sizeof(float)) != hipSuccess || hipMalloc(&de, n * sizeof(float)) != hipSuccess ||
        hipMalloc(&dl, n * sizeof(float)) != hipSuccess) { std::printf("hipMalloc failed\n"); return 1; }
    if (hipMemcpy(dx, x.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { std::printf("copy failed\n"); return 1; }
    eval<<<(n + 255) / 256, 256>>>(dx, de, dl, n);
    if (hipMemcpy(ex.data(), de, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(lg.data(), dl, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { std::printf("kernel or copy failed\n"); return 1; }
    double we = 0.0, wn = 0.0, wl = 0.0;                      // expf: over the whole range, and where the result is a normal number
    for (int i = 0; i < n; ++i) {
        const double r = std::exp((double)x[i]), u = ulps(ex[i], r);
        if (u > we) we = u;
        if (r >= 1.1754943508222875e-38 && u > wn) wn = u;
        const double v = ulps(lg[i], std::log((double)x[n + i]));
        if (v > wl) wl = v;
    }
    std::printf("expf on [-140, 0], %d arguments: worst error %.3f ulp where the result is normal, %.3f ulp (of the least subnormal) overall\n", n, wn, we);
    std::printf("logf on [2^-5, 1], %d arguments: worst error %.3f ulp\n", n, wl);
    (void)hipFree(dx); (void)hipFree(de); (void)hipFree(dl);
    return 0;
}
