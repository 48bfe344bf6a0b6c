// CPU: the argument rules of lsnf_mala_step, lsnf_reverse_mala_step, lsnf_hmc_step and lsnf_reverse_hmc_step under the host sanitizers.  Refused
// calls only:
// every refusal returns before any HIP call, so no device is needed and the addresses below are never dereferenced.
//
//   cd latent-space-normalizing-flow_amd/csrc && make                         # the plain objects
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 $S -c lsnf_api.hip -o _build/lsnf_api_san.o
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 $S -c ../../tools/chain_rules_sanitized.cpp -o _build/chain_rules_san.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined _build/chain_rules_san.o _build/lsnf_api_san.o \
//         $(ls _build/*.o | grep -v -e lsnf_api -e _san) -o _build/chain_rules_sanitized && _build/chain_rules_sanitized
//
// Exit status 0 and "N refusals, 0 unexpected" when every call was refused with LSNF_E_ARG and a message naming its entry point; a
// sanitizer report ends the program with its own status.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "../include/lsnf_flow_mcmc.h"

namespace {
float* at(int i, unsigned off = 0) { return reinterpret_cast<float*>(0x10000ul * (i + 1) + off); }
struct Args {                            // a call every rule lets through, over which one field is changed at a time
    int nz = 128, width = 64, depth = 5, B = 4;
    float *plan = at(0), *point = at(1), *z_out = at(2), *z_saved = at(3), *act_saved = at(4), *ll_prop = at(5), *grad_g = at(6), *energy_g = at(7),
          *acc = at(8), *grad_acc = at(9), *u_acc = at(10), *mom = at(11), *kin0 = at(12), *noise = at(13), *uniform = at(14), *next = at(15),
          *accept_out = nullptr, *log_alpha_out = nullptr;
    const LsnfRng* rng = nullptr;
    float step = 0.9f;
    unsigned flags = 0;
};
int mala(const Args& a) {
    return lsnf_mala_step(a.plan, a.nz, a.width, a.depth, 1, a.B, a.point, a.z_out, a.z_saved, a.act_saved, a.ll_prop, a.grad_g, a.energy_g, a.acc,
                          a.grad_acc, a.u_acc, a.noise, a.uniform, a.rng, a.step, a.flags, a.next, a.accept_out, a.log_alpha_out, nullptr);
}
int rmala(const Args& a) {
    return lsnf_reverse_mala_step(a.plan, a.nz, a.width, a.depth, 1, a.B, a.point, a.z_saved, a.act_saved, a.grad_g, a.energy_g, a.acc, a.grad_acc,
                                  a.u_acc, a.noise, a.uniform, a.rng, a.step, a.flags, a.next, a.accept_out, a.log_alpha_out, nullptr);
}
int hmc(const Args& a) {
    return lsnf_hmc_step(a.plan, a.nz, a.width, a.depth, 1, a.B, a.point, a.z_out, a.z_saved, a.act_saved, a.ll_prop, a.grad_g, a.energy_g, a.acc,
                         a.grad_acc, a.u_acc, a.mom, a.kin0, a.noise, a.uniform, a.rng, a.step, a.flags, a.next, a.accept_out, a.log_alpha_out,
                         nullptr);
}
int rhmc(const Args& a) {
    return lsnf_reverse_hmc_step(a.plan, a.nz, a.width, a.depth, 1, a.B, a.point, a.z_saved, a.act_saved, a.grad_g, a.energy_g, a.acc, a.grad_acc,
                                 a.u_acc, a.mom, a.kin0, a.noise, a.uniform, a.rng, a.step, a.flags, a.next, a.accept_out, a.log_alpha_out, nullptr);
}
}  // namespace

int main() {
    const LsnfRng ok = {1ull, 0ull, nullptr, 0ll}, neg = {1ull, 0ull, nullptr, -1ll};
    const LsnfRng odd = {1ull, 0ull, reinterpret_cast<const unsigned long long*>(0x30004ul), 0ll};
    struct Entry { const char* name; int (*call)(const Args&); unsigned unknown, inner; } const entries[] = {
        {"lsnf_mala_step", mala, 2u, 0u}, {"lsnf_reverse_mala_step", rmala, 2u, 0u}, {"lsnf_hmc_step", hmc, 4u, LSNF_HMC_INNER},
        {"lsnf_reverse_hmc_step", rhmc, 4u, LSNF_HMC_INNER}};
    int refusals = 0, unexpected = 0;
    for (const Entry& e : entries) {
        auto refused = [&](const char* what, Args a) {
            const int rc = e.call(a);
            const char* msg = lsnf_last_error();
            const bool fine = rc == LSNF_E_ARG && !strncmp(msg, e.name, strlen(e.name)) && strstr(msg, what);
            printf("%s %-40s rc %d  %s\n", fine ? "  " : "!!", what, rc, msg);
            ++refusals; unexpected += !fine;
        };
        for (int k = 0; k < (e.inner ? 2 : 1); ++k) {     // (the HMC entries: the rules again for an inner call, where they apply)
            const unsigned phase = k ? e.inner : 0u;
            Args base;
            base.flags = phase;
            if (phase) base.noise = base.uniform = nullptr;
            Args a = base;
            a.B = -1; refused("out of range", a);
            a = base; a.step = NAN; refused("step_size", a);
            a = base; a.B = 0; a.step = 0.0f; refused("step_size", a);
            a = base; a.flags |= e.unknown; refused("unknown flag", a);
            a = base; a.acc = a.grad_g; refused("must not alias grad_g", a);
            a = base; a.next = a.u_acc; refused("must not alias", a);
            a = base; a.accept_out = a.log_alpha_out = at(16); refused(phase ? "must be NULL" : "must not alias", a);
            a = base; a.plan = nullptr; refused("plan is required", a);
            a = base; a.act_saved = nullptr; refused("act_saved is required", a);
            a = base; a.u_acc = nullptr; refused("u_acc is required", a);
            a = base; a.z_saved = nullptr; refused("z_saved is required", a);
            a = base; a.plan = at(0, 4); refused("plan must be 16-byte", a);
            a = base; a.act_saved = at(4, 8); refused("act_saved must be 16-byte", a);
            a = base; a.grad_g = at(6, 2); refused("grad_g must be 4-byte", a);
            a = base; a.next = at(15, 2); refused("must be 4-byte", a);
            a = base; a.rng = &ok; refused(phase ? "rng is not taken" : "not both", a);
            if (phase) {
                a = base; a.next = nullptr; refused("is required (NULL) with", a);
                a = base; a.noise = at(13); refused("noise is not taken", a);
                a = base; a.flags |= LSNF_HMC_INIT; refused("exclude each other", a);
                continue;
            }
            a = base; a.noise = nullptr; a.rng = &ok; refused("uniform tensor or an rng", a);
            a = base; a.noise = a.uniform = nullptr; a.rng = &neg; refused("row0", a);
            a = base; a.noise = a.uniform = nullptr; a.rng = &odd; refused("offset_dev", a);
            a = base; a.uniform = nullptr; refused("uniform is required", a);
            a = base; a.noise = nullptr; refused("noise is required", a);
            a = base; a.next = nullptr; refused("noise goes with", a);
            a = base; a.log_alpha_out = at(16, 1); refused("log_alpha_out must be 4-byte", a);
        }
    }
    printf("%d refusals, %d unexpected\n", refusals, unexpected);
    return unexpected ? 1 : 0;
}
