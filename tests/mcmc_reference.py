"""fp64 numpy restatements of the two MCMC-densification formulas (include/gsr/gsr_train.h:
gsr_mcmc_relocate, gsr_mcmc_noise), for the tests to compare the kernels against.

The relocation is upstream's DOUBLE sum with math.comb, not the collapsed one the kernel evaluates, so
that the hockey-stick identity is tested rather than assumed; `relocation_denominator_collapsed` is
the kernel's form.  The noise builds R and Sigma in fp64 from the fp32 inputs."""
from __future__ import annotations

import math

import numpy as np

MAX_RATIO = 51
OPACITY_MAX = 1.0 - 2.0 ** -24


def clamp_ratio(n: int) -> int:
    return min(max(int(n), 1), MAX_RATIO)


def relocation_x(o: float, n: int) -> float:
    return 1.0 - (1.0 - float(o)) ** (1.0 / n)


def relocation_denominator(x: float, n: int) -> float:
    """D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1), in upstream's order."""
    d = 0.0
    for i in range(1, n + 1):
        for k in range(i):
            d += math.comb(i - 1, k) * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1)
    return d


def relocation_denominator_collapsed(x: float, n: int) -> float:
    """The same D by sum_{i=k+1..N} C(i-1, k) = C(N, k+1): O(N)."""
    return sum(math.comb(n, k + 1) * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1) for k in range(n))


def relocate(opacities, scales, ratios, min_opacity: float):
    """-> (new_opacities (n,), new_scales (n, 3)) in float64 from float32 inputs."""
    o = np.asarray(opacities, np.float32).astype(np.float64)
    s = np.asarray(scales, np.float32).astype(np.float64).reshape(-1, 3)
    new_o, new_s = np.empty_like(o), np.empty_like(s)
    for i in range(o.shape[0]):
        n = clamp_ratio(ratios[i])
        x = relocation_x(o[i], n)
        new_s[i] = (o[i] / relocation_denominator(x, n)) * s[i]
        new_o[i] = min(max(x, float(np.float32(min_opacity))), OPACITY_MAX)
    return new_o, new_s


def rotation(q):
    """general.build_rotation in float64: q (P, 4), w first, normalised by max(|q|, 1e-12)."""
    q = np.asarray(q, np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3)


def noise_gate(opac_raw):
    o = 1.0 / (1.0 + np.exp(-np.asarray(opac_raw, np.float64).reshape(-1)))
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(100.0 * (o - 0.005)))


def noise_displacement(scale_raw, rot_raw, opac_raw, noise, strength: float):
    """R diag(s^2) R^T (noise * gate * strength), (P, 3) float64, from float32 inputs."""
    s = np.exp(np.asarray(scale_raw, np.float32).astype(np.float64))
    R = rotation(np.asarray(rot_raw, np.float32))
    gate = noise_gate(np.asarray(opac_raw, np.float32))
    sigma = R @ (s[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))
    v = np.asarray(noise, np.float32).astype(np.float64) * gate[:, None] * float(np.float32(strength))
    return np.einsum("pij,pj->pi", sigma, v)
