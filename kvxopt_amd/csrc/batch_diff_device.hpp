// What k_qp_batch_diff (qp_batch_diff.hip) and k_coneqp_batch_diff (coneqp_batch_diff.hip) have as the same text and can share
// without a change of their code objects.
#pragma once
#include "batch_device.hpp"

namespace kvx {
namespace batchdev {

// row i of the symmetric matrix whose lower triangle is in HBM, times the LDS vector v
__device__ __forceinline__ double sym_row_dot(const double *__restrict__ Q, int n, int i, const double *v)
{
    double t = 0.0;
    for (int j = 0; j < n; j++) t += (j <= i ? Q[i + j * n] : Q[j + i * n]) * v[j];
    return t;
}

}  // namespace batchdev
}  // namespace kvx
