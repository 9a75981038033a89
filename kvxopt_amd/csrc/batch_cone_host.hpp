// What the host entries of the kernels with 'l', 'q' and 's' rows share (conelp_batch_api.cpp, coneqp_batch_api.cpp,
// coneqp_batch_diff_api.cpp and the query kvx_coneqp_batch_diff_lds_bytes): the limits of the cone with their texts, in the order
// the entries refuse in, and the placement of the cone in the kernel's arguments.  An entry keeps what comes after: conelp's rank
// condition, the derivative's options, the LDS refusal, the pointers and the strides.
#pragma once
#include "batch_host.hpp"
#include "conelp_batch.hpp"

namespace kvx {
namespace batchhost {

// nullptr when B, n, ml, nq, q, ns, m, the orders, N = ml + sum(q) + sum(m^2) and p are within the limits of the cone kernels,
// else the text of the first one that is not; *N on success.
inline const char *cone_limits(int64_t B, int n, int ml, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m, int p, int64_t *N)
{
    if (B < 1 || B > 2147483647) return "1 <= B <= 2147483647 is required";
    if (n < 1 || n > CONEB_MAX_N) return "1 <= n <= 64 is required";
    if (ml < 0 || ml > CONEB_MAX_ROWS) return "0 <= ml <= 384 is required";
    if (nq < 0 || nq > CONEB_MAX_NQ) return "0 <= nq <= 128 is required";
    if (nq > 0 && !q) return "the cone orders q are NULL";
    if (ns < 0 || ns > CONEB_MAX_NS) return "0 <= ns <= 32 is required";
    if (ns > 0 && !m) return "the block orders m are NULL";
    *N = ml;
    for (int64_t k = 0; k < nq; k++) {
        if (q[k] < 1 || q[k] > CONEB_MAX_ROWS) return "every cone order is at least 1 and at most 384";
        *N += q[k];
    }
    for (int64_t k = 0; k < ns; k++) {
        if (m[k] < 1 || m[k] > CONEB_MAX_M) return "every block order is at least 1 and at most 16";
        *N += m[k] * m[k];
    }
    if (*N < 1 || *N > CONEB_MAX_ROWS) return "1 <= N = ml + sum(q) + sum(m^2) <= 384 is required";
    if (p < 0 || p > n) return "0 <= p <= n is required";
    return nullptr;
}

// the cone into the kernel's arguments; the orders are in range (cone_limits)
template <class Args>
void place_cone(Args &a, int64_t nq, const int64_t *q, int64_t ns, const int64_t *m)
{
    a.nq = (int)nq;
    a.ns = (int)ns;
    a.Ms = a.ml;
    for (int64_t k = 0; k < CONEB_MAX_NQ; k++) a.q[k] = k < nq ? (unsigned short)q[k] : 0;
    for (int64_t k = 0; k < CONEB_MAX_NS; k++) a.m[k] = k < ns ? (unsigned char)m[k] : 0;
    for (int64_t k = 0; k < nq; k++) a.Ms += (int)q[k];
    a.N = a.Nd = a.Np = a.Ms;
    for (int64_t k = 0; k < ns; k++) {
        a.N += (int)(m[k] * m[k]);
        a.Nd += (int)m[k];
        a.Np += (int)((m[k] * (m[k] + 1)) / 2);
    }
}

}  // namespace batchhost
}  // namespace kvx
