// lsnf_small3_rhmca.hip -- Hamiltonian Monte Carlo in the flow's base space with a likelihood temperature per row, a resampling move
// between the rows of a group and the group's next temperature searched in the annealing call (lsnf_reverse_hmc_step_schedule,
// include/lsnf_flow_mcmc.h): the latency bf16x3 reverse-backward of lsnf_small3_rbwd.hip (lsnf_small3_rbwd_kernel.h) with the leapfrog
// tail of lsnf_rhmc_tail.h at its SCHEDULE level as the output section.
#include <stdlib.h>
#include "lsnf_rhmc_tail.h"
#include "lsnf_hmc_launch.h"

namespace {
using F = LsnfHmcLevel<LSNF_LEVEL_SCHEDULE>;
}
#define LSNF_S3R_KERNEL lsnf_small3_rhmca_kernel
#define LSNF_S3R_ARGS Small3RhmcScheduleArgs
#define LSNF_S3R_TAIL small3_rhmc_tail<F, HT, ST>(a, g1, g2, y2, sample, live, row, GTP, has1, nt1, ft1, wave, g, n, vec4); return;
#include "lsnf_small3_rbwd_kernel.h"

// st: lsnf_small3_reverse_backward_st of the call
hipError_t lsnf_launch_small3_reverse_hmc_schedule(const LsnfReverseHmcScheduleCall& c, int st) {
    if (!lsnf_rhmc_call_ok<F>(c)) return hipErrorInvalidValue;                   // (a selection bug)
    Small3RhmcScheduleArgs a;
    lsnf_fill_rhmc<F>(a, c);
    return lsnf_with_cfg<Small3RbwdCfg>(c.g, [&](auto cfg) {
        return lsnf_with_st(st, [&](auto s) -> hipError_t {
            using C = decltype(cfg);
            constexpr int ST = decltype(s)::value;
            if constexpr (!small3_rbwd_built<C, ST>) return hipErrorInvalidValue;     // (a selection bug)
            else return lsnf_launch_kernel<lsnf_small3_rhmca_kernel<C, ST, false>>(lsnf_grid(a.B, ST * S3_SAMPLES), 256,
                                                                                  (size_t)Small3RbwdLds<C, ST>::L_END * sizeof(float), c.stream, a);
        });
    });
}
