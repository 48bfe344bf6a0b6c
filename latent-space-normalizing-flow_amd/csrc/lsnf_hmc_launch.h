// lsnf_hmc_launch.h -- host: what the launchers of the fourteen HMC translation units refuse and how they fill their kernels' arguments,
// stated once for every level (lsnf_hmc_level.h) and both spaces.
#pragma once
#include "lsnf_launch.h"
#include "lsnf_hmc_level.h"

// ---- what a launcher refuses (a selection bug: the entries of lsnf_api.hip refuse all of it with a message first) ----
// the levels' part, the same in both spaces; c: the level's call descriptor of either space, rng_on: the call draws in-kernel
template <class F, class C>
static inline bool lsnf_hmc_levels_ok(const C& c, bool rng_on) {
    const unsigned f = c.chain.flags;
    const bool inner = (f & 2u) != 0, adapt = (f & 4u) != 0, fold = (f & 16u) != 0, anneal = (f & 64u) != 0;
    if (!c.mom || !c.kin0) return false;
    if constexpr (F::ROWS)
        if (!c.step_rows || (adapt != (c.adapt != nullptr)) || (adapt && (f & 3u)) || ((f & 8u) && !adapt)) return false;
    if constexpr (F::METRIC)
        if (!c.scale || (fold && (f & 3u)) || ((f & 32u) && !fold) || (fold != (c.mean != nullptr)) || (fold != (c.m2 != nullptr)) ||
            (fold != (c.count != nullptr)))
            return false;
    if constexpr (F::TEMPER)
        if (!c.beta_rows || !c.like_grad_acc || !c.like_u_acc || (anneal && inner) || (anneal != (c.beta_next != nullptr)) ||
            (anneal != (c.log_w != nullptr)))
            return false;
    if constexpr (F::EXCHANGE) {
        const bool swap = (f & 128u) != 0;
        const bool ladder_ok = (c.ladder == 2 || c.ladder == 4 || c.ladder == 8 || c.ladder == 16) && c.B % c.ladder == 0;
        if ((swap && (!ladder_ok || (f & (1u | 2u | 4u | 16u | 32u | 64u)))) || ((f & 256u) && !swap) ||
            (!swap && (c.swap_uniform || c.swap_out || c.log_swap_out)) ||
            (swap && (rng_on ? c.swap_uniform != nullptr : c.swap_uniform == nullptr)))
            return false;
    }
    if constexpr (F::SCHEDULE) {                                       // (`group` serves SCHEDULE and RESAMPLE)
        const bool group_ok = (c.group == 2 || c.group == 4 || c.group == 8 || c.group == 16) && c.B % c.group == 0;
        if ((f & 1024u) && (!group_ok || !anneal || inner || (f & (4u | 16u | 32u)) || !(c.cess_frac > 0.0f && c.cess_frac < 1.0f) ||
                            !(c.min_step >= 0.0f && c.min_step <= 3.4028234663852886e38f)))
            return false;
    }
    if constexpr (F::RESAMPLE) {
        const bool resample = (f & 512u) != 0;
        const bool group_ok = (c.group == 2 || c.group == 4 || c.group == 8 || c.group == 16) && c.B % c.group == 0;
        if ((f & (128u | 256u)) || (resample && (!group_ok || !anneal || (f & (1u | 2u | 4u | 16u | 32u)))) ||
            (!resample && (c.resample_uniform || c.ancestor_out || c.ess_out)) ||
            (resample && (rng_on ? c.resample_uniform != nullptr : c.resample_uniform == nullptr)))
            return false;
    }
    return true;
}
// z space: c is LsnfHmcCall or what derives from it
template <class F, class C>
static inline bool lsnf_hmc_call_ok(const C& c) {
    const bool inner = (c.chain.flags & 2u) != 0;
    if (!c.act_saved || !c.lv || c.dump || c.g_z_in || c.B < 1 || (c.lv->rng.enabled && (c.lv->noise || c.chain.uniform)) ||
        (inner && (!c.lv->z_new || c.lv->noise || c.chain.uniform || c.lv->rng.enabled || (c.chain.flags & 1u))))
        return false;
    return lsnf_hmc_levels_ok<F>(c, c.lv->rng.enabled != 0);
}
// base space: c is LsnfReverseHmcCall or what derives from it
template <class F, class C>
static inline bool lsnf_rhmc_call_ok(const C& c) {
    const bool inner = (c.chain.flags & 2u) != 0;
    if (!c.act_saved || !c.chain.acc || !c.chain.grad_acc || !c.chain.u_acc || c.g_z_in || c.g_norm || c.eps_norm || c.B < 1 ||
        (c.rng.enabled && (c.noise || c.chain.uniform)) || (!inner && c.eps_new && !c.noise && !c.rng.enabled) ||
        (inner && (!c.eps_new || c.noise || c.chain.uniform || c.rng.enabled || (c.chain.flags & 1u))))
        return false;
    return lsnf_hmc_levels_ok<F>(c, c.rng.enabled != 0);
}

// ---- the kernel arguments of a level from its call descriptor ----
template <class F, class A, class C>
static inline void lsnf_fill_hmc_levels(A& a, const C& c) {
    a.mom = c.mom; a.kin0 = c.kin0;
    if constexpr (F::ROWS) { a.step_rows = c.step_rows; a.adapt = c.adapt; a.da = c.da; }
    if constexpr (F::METRIC) { a.scale = c.scale; a.mean = c.mean; a.m2 = c.m2; a.count = c.count; a.reg = c.reg; }
    if constexpr (F::TEMPER) {
        a.beta_rows = c.beta_rows; a.beta_next = c.beta_next; a.like_grad_acc = c.like_grad_acc; a.like_u_acc = c.like_u_acc; a.log_w = c.log_w;
    }
    if constexpr (F::EXCHANGE) { a.ladder = c.ladder; a.swap_uniform = c.swap_uniform; a.swap_out = c.swap_out; a.log_swap_out = c.log_swap_out; }
    if constexpr (F::RESAMPLE) {
        a.group = c.group; a.ess_frac = c.ess_frac; a.resample_uniform = c.resample_uniform; a.ancestor_out = c.ancestor_out; a.ess_out = c.ess_out;
    }
    if constexpr (F::SCHEDULE) { a.cess_frac = c.cess_frac; a.min_step = c.min_step; }
}
// z space: Small3HmcArgs or what derives from it
template <class F, class A, class C>
static inline void lsnf_fill_hmc(A& a, const C& c) {
    lsnf_fill_mala(a, c);
    lsnf_fill_hmc_levels<F>(a, c);
}
// base space: Small3RhmcArgs or what derives from it (the upstream gradient is grad_g; a per-row level does not read `step`)
template <class F, class A, class C>
static inline void lsnf_fill_rhmc(A& a, const C& c) {
    a.panels = c.plan + c.g.off_b3b_panels;
    a.tpanels = c.plan + c.g.off_t3b_panels;
    a.z_out = c.z_out; a.z_saved = c.z_saved; a.act_saved = c.act_saved; a.g_x = c.grad_g; a.g_obj = nullptr; a.g_z_in = nullptr;
    a.B = c.B; a.nz = c.g.nz; a.half = c.g.half; a.depth = c.g.depth; a.vec4 = c.vec4;
    a.noise = c.noise; a.eps_new = c.eps_new; a.g_norm = nullptr; a.eps_norm = nullptr; a.step = F::ROWS ? 0.0f : c.step; a.rng = c.rng;
    a.eps_acc = c.chain.acc;
    lsnf_fill_chain(a, c.chain);
    lsnf_fill_hmc_levels<F>(a, c);
}
