// k_coneqp_batch: one workgroup (256 threads, four wavefronts) carries one small dense cone QP from its starting point to its
// status (coneqp_batch.hpp).  It is coneqp_member (batch_coneqp.hpp) on the cone K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ... of
// batch_cone.hpp, the cone code k_conelp_batch carries, included below into this file's anonymous namespace: the rows, the
// tables, the work per kind of row and the assembly of S over staged rows of W^-T G are described in conelp_batch.hip.  What
// this kernel adds to the cone is in the "coneqp" parts of that header: S starts from the lower triangle of P, the right-hand
// side takes rz whole, and combine knows no dtau.
//
// LDS.  The member has no x1, y1, z1 and no W^-T h: the layout (batch_coneqp_layout.hpp) is conelp's without those four vectors, so
// it is smaller at every shape.  P, q, G, h, A, b are read from HBM / L2 as k_qp_batch reads them.
//
// Sums over all rows have the fixed order of batch_device.hpp.  Every loop is bounded by maxiters, n, N, p, nq, ns, q_k, m_k or
// CONEB_SWEEPS.  A block that is not finite is not iterated on.
#include "coneqp_batch.hpp"
#include "batch_coneqp.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == CONEB_THREADS, "the shared helpers are written for the workgroup of k_coneqp_batch");
static_assert(CONEB_MAX_M * CONEB_MAX_M <= NT, "a thread per entry of a block");
static_assert(CONEQP_NSTAT == CONEQPB_NSTAT, "the stats of coneqp_member");
#include "batch_cone.hpp"

#include "batch_coneqp_layout.hpp"

__global__ void __launch_bounds__(CONEB_THREADS) k_coneqp_batch(ConeqpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int ml = a.ml, nq = a.nq, ns = a.ns, Ms = a.Ms;
    const QpLayout L = qp_layout(a.n, ml, Ms, a.N, a.Nd, a.Np, nq, ns, a.p);
    Member M;
    conelp_data(M, a, a.N);
    M.P = a.P + (int64_t)blockIdx.x * a.sP;
    M.ml = ml; M.nq = nq; M.ns = ns; M.Ms = Ms; M.Nd = a.Nd; M.Np = a.Np; M.ldn = L.ldn; M.ldp = L.ldp;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K; M.w = lds + L.w; M.g = lds + L.g;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry;
    M.x1 = nullptr; M.y1 = nullptr; M.z1 = nullptr; M.th = nullptr;      // conelp's; nothing coneqp_member calls reads them
    M.s = lds + L.s; M.z = lds + L.z; M.ds = lds + L.ds; M.dz = lds + L.dz; M.rz = lds + L.rz; M.ws3 = lds + L.ws3;
    M.tw = lds + L.tw; M.r = lds + L.r; M.rti = lds + L.rti;
    M.lm = lds + L.lm; M.d = lds + L.d; M.di = lds + L.di; M.beta = lds + L.beta; M.sgs = lds + L.sgs; M.sgz = lds + L.sgz;
    M.wa = lds + L.wk; M.wb = M.wa + MM; M.wc = M.wb + MM; M.wd = M.wc + MM; M.nrm = lds + L.nrm;
    M.red = lds + L.red;
    M.off = reinterpret_cast<int *>(lds + L.off);
    M.cone = reinterpret_cast<unsigned short *>(lds + L.cone);
    M.bo = reinterpret_cast<int *>(lds + L.blk); M.bl = M.bo + (ns + 1);
    M.flag = reinterpret_cast<int *>(lds + L.flag);
    unsigned short *prow = reinterpret_cast<unsigned short *>(lds + L.prow), *pmir = reinterpret_cast<unsigned short *>(lds + L.pmir);
    M.prow = prow; M.pmir = pmir;

    cone_tables(M, a, prow, pmir);
    coneqp_member(Cone{M}, a, a.correction != 0);
}

}  // namespace

size_t coneqp_batch_lds_bytes(int n, int ml, int nq, const unsigned short *q, int ns, const unsigned char *m, int p)
{
    const Sizes z = sizes(ml, nq, q, ns, m);
    return (size_t)qp_layout(n, ml, z.Ms, z.N, z.Nd, z.Np, nq, ns, p).total * sizeof(double);
}

hipError_t launch_coneqp_batch(hipStream_t st, const ConeqpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_coneqp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_coneqp_batch<<<dim3((unsigned)a.B), dim3(CONEB_THREADS), coneqp_batch_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
