// rbf_device.hpp -- the kernel forms of the scaled RBF closure, r2 -> phi and the factor of d_k in dphi/dxs_k, written once for
// rbf.hip and rbf_fit.hip (each sums r2 in its own order; `kind` is their template argument).  The `centre` lambda of
// rom_rbf_fused.hip repeats them with its run-time kind: sharing them changed that kernel's generated code.
#pragma once
#include "../../include/burgers_hip.h"
namespace bg {
__device__ __forceinline__ double rbf_value(int kind, double eps2, double r2)
{
    return kind == BG_RBF_GAUSSIAN ? exp(-eps2 * r2) : 1.0 / sqrt(1.0 + eps2 * r2);        // else (1 + eps^2 r2)^(-1/2)
}
__device__ __forceinline__ double rbf_value_coef(int kind, double eps2, double r2, double& coef)
{
    const double p = rbf_value(kind, eps2, r2);
    coef = kind == BG_RBF_GAUSSIAN ? -2.0 * eps2 * p : -eps2 * (p * p * p);                // dphi/dxs_k = coef d_k
    return p;
}
}  // namespace bg
