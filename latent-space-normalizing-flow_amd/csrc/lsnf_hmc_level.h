// lsnf_hmc_level.h -- the levels of the Hamiltonian Monte Carlo steps (include/lsnf_flow_mcmc.h) as a compile-time description, for the
// two tails (lsnf_hmc_tail.h in z, lsnf_rhmc_tail.h in the flow's base space), their fourteen translation units and the launchers'
// rules (lsnf_hmc_launch.h).
//
// A level is what a step has on top of the scalar one.  The ladder is linear up to TEMPERED; EXCHANGE and RESAMPLE both stand on
// TEMPERED and not on each other, SCHEDULE stands on RESAMPLE (the call descriptors of lsnf_launch.h and the kernels' argument structs
// inherit the same way):
//   ROWS       a step per row (step_rows; `step` is not read) and its dual-averaging adaptation (ADAPT, ADAPT_LAST)
//   METRIC     a diagonal metric per row (scale) and its windowed adaptation (METRIC_FOLD, METRIC_CLOSE)
//   TEMPER     a likelihood temperature per row (beta_rows), the likelihood's part of the kept state, the annealing move (ANNEAL)
//   EXCHANGE   the replica-exchange move between neighbouring rows of a ladder (SWAP, SWAP_ODD)
//   RESAMPLE   the resampling move between the rows of a group on an annealing end call (RESAMPLE)
//   SCHEDULE   the group's next temperature searched from its particles on an annealing call (SCHEDULE, lsnf_schedule.h)
// A kernel or a launcher of level F touches the members of its level's structs only: everything a lower level lacks stands
// under `if constexpr (F::...)`.
#pragma once

enum LsnfHmcLevelId { LSNF_LEVEL_SCALAR, LSNF_LEVEL_ROWS, LSNF_LEVEL_METRIC, LSNF_LEVEL_TEMPERED, LSNF_LEVEL_EXCHANGE, LSNF_LEVEL_RESAMPLE, LSNF_LEVEL_SCHEDULE };
template <LsnfHmcLevelId L>
struct LsnfHmcLevel {
    static constexpr bool ROWS = L >= LSNF_LEVEL_ROWS, METRIC = L >= LSNF_LEVEL_METRIC, TEMPER = L >= LSNF_LEVEL_TEMPERED;
    static constexpr bool EXCHANGE = L == LSNF_LEVEL_EXCHANGE, RESAMPLE = L >= LSNF_LEVEL_RESAMPLE, SCHEDULE = L == LSNF_LEVEL_SCHEDULE;
};
