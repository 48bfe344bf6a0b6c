"""Fused prior sampling (`lsnf_sample`) restated on the two oracles (shared by test_sample_cpu.py and test_gpu_sample.py; not a
test module):

    eps64        = T * oracle.philox_oracle.langevin_noise(B, nz, seed, offset, row0)         the drawn latent rows
    x64, obj64   = oracle.flow_oracle.flow_reverse(params64, eps64, 0)                        obj64 = objective_out = -logdet_f(x)
    ll64         = -0.5 * sum_c eps64^2 + log(2 pi) - obj64                                   log p(x) under the flow prior

`ll` is `oracle.flow_oracle.log_prob(z1 = eps, logdet = -obj)`: the ll_out that lsnf_forward documents, evaluated at x."""
import math

import torch

from oracle import flow_oracle as O
from oracle.philox_oracle import langevin_noise


def draws(B, nz, seed, offset=0, row0=0, temperature=1.0):
    """(B, nz) float64: the rows lsnf_sample draws for global rows row0 .. row0 + B - 1."""
    return torch.from_numpy(langevin_noise(B, nz, seed, offset, row0)) * float(temperature)


def ll(eps, obj):
    """log p(x) from the drawn rows and the reverse's objective_out, in the dtype of its inputs."""
    return -0.5 * (eps ** 2).flatten(1).sum(-1) + math.log(2.0 * math.pi) - obj


def flow_at(p, eps):
    """(x64, obj64, ll64) of the float64 oracle at the given latent rows (any dtype; evaluated as float64)."""
    e = eps.double()
    x, negobj = O.flow_reverse(O.to_dtype(p, torch.float64), e, torch.zeros(e.shape[0], dtype=torch.float64))
    return x, -negobj, ll(e, -negobj)


def sample(p, B, nz, seed, offset=0, row0=0, temperature=1.0):
    """(eps64, x64, obj64, ll64): the whole call in float64."""
    e = draws(B, nz, seed, offset, row0, temperature)
    return (e,) + flow_at(p, e)
