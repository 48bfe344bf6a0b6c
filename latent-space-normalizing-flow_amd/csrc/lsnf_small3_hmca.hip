// lsnf_small3_hmca.hip -- Hamiltonian Monte Carlo in z with a likelihood temperature per row, a resampling move between the rows of a
// group and the group's next temperature searched in the annealing call (lsnf_hmc_step_schedule, include/lsnf_flow_mcmc.h): the
// latency bf16x3 backward of lsnf_small3_bwd.hip (lsnf_small3_bwd_kernel.h) with the leapfrog tail of lsnf_hmc_tail.h at its SCHEDULE
// level as the output section.
#include <stdlib.h>
#include "lsnf_hmc_tail.h"
#include "lsnf_hmc_launch.h"

namespace {
using F = LsnfHmcLevel<LSNF_LEVEL_SCHEDULE>;
}
#define LSNF_S3B_KERNEL lsnf_small3_hmca_kernel
#define LSNF_S3B_ARGS Small3HmcScheduleArgs
#define LSNF_S3B_TAIL small3_hmc_tail<F, HT, ST>(a, gx1, gx2, sample, live, row, RED, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_bwd_kernel.h"

// st: lsnf_small3_backward_st of the call
hipError_t lsnf_launch_small3_hmc_schedule(const LsnfHmcScheduleCall& c, int st) {
    if (!lsnf_hmc_call_ok<F>(c)) return hipErrorInvalidValue;                    // (a selection bug)
    Small3HmcScheduleArgs a;
    lsnf_fill_hmc<F>(a, c);
    return lsnf_with_cfg<Small3BwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) -> hipError_t {
            using C = decltype(cfg);
            constexpr int ST = decltype(s)::value;
            if constexpr (!small3_bwd_built<C, ST>) return hipErrorInvalidValue;      // (a selection bug)
            else return lsnf_launch_kernel<lsnf_small3_hmca_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256,
                                                                                 (size_t)Small3BwdLds<C, ST>::L_END * sizeof(float), c.stream, a);
        });
    });
}
