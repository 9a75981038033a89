// k_conelp_batch: one workgroup (256 threads, four wavefronts) carries one small dense cone program from its starting point to its
// status or its infeasibility certificate (conelp_batch.hpp).  It is conelp_member (batch_conelp.hpp) on the cone
// K = R^ml_+ x Q^{q_0} x ... x S^{m_0}_+ x ... with all three kinds at once.  The policy below is the composition of the two that
// k_socp_batch and k_sdp_batch carry: per operation the orthant functions of batch_conelp.hpp / batch_kkt.hpp on the 'l' rows,
// the 'q' operations of batch_cone_q.hpp on the 'q' rows and the 's' operations of batch_cone_s.hpp on the 's' rows (the
// reference's misc.compute_scaling / update_scaling, misc.py:284-419, 444-634, and scale, scale2, sprod, sinv, sdot,
// max_step of misc_solvers.c), strung together as cone.py::_ConeEngine strings them.
//
// The cone's device code is batch_cone.hpp, included below into this file's anonymous namespace and shared with k_coneqp_batch:
// the layout, the member, W, the assembly of S and the policy.  The 'q' and the 's' operations it strings together are
// batch_cone_q.hpp and batch_cone_s.hpp, the text k_socp_batch and k_sdp_batch run as well, each kernel with an internal copy
// (DESIGN 16, 17, 18).  What a member of this kernel computes on a row of a kind is what the sibling computes on it.
//
// Rows.  A vector of the cone has N = ml + sum q_k + sum m_k^2 entries: the 'l' rows, the cones, then every 's' block as its full
// symmetric m x m matrix, column-major with leading dimension m; both triangles are written from one value.  G and h are read
// through the tables of the Np = ml + sum q_k + sum m_k (m_k + 1) / 2 packed rows: prow[j], the row of the j-th packed entry, and
// pmir[j], the row of its mirror image.  An 'l' or 'q' row is its own mirror and has weight 1; an off-diagonal entry of a block
// counts twice in G'z and in the inner product.  The upper triangles of G and h are never read.  lmbda has
// Nd = ml + sum q_k + sum m_k entries.
//
// Work.  A cone belongs to one wavefront at a time (lanes along its rows, xor butterfly), a block to the workgroup, one block
// after the other (a thread per entry; sixteen lanes per column pair in the one-sided Jacobi, two matrices between the same
// barriers).  The loops over cones have no barrier inside, the loops over blocks are the same for every thread.
//
// S = Gs'Gs with Gs = W^-T G is assembled from staged rows of Gs, at most 32 at a time, in the region X and K take after the
// factorisation, which holds at once the 32 staged rows, the 16 rows w of the block column being staged and the ring of 33 row
// vectors g_k = (J v_k)'G_k.  The 'l' and 'q' rows go in tiles of 32 from row 0, as k_socp_batch stages them: a cone's g_k is
// computed when the tile with its first row is staged and kept while later tiles stage the rest of the cone, so a cone may
// straddle any number of tile boundaries.  A full tile is added to S at once; the partly filled tile at the end of the 'q'
// rows stays, and the block columns of the 's' blocks are appended to it as k_sdp_batch appends them to its last 'l' tile.
//
// Sums over all rows have the fixed order of batch_device.hpp.  Every loop of this file is bounded by n, N, nq, ns, q_k, m_k or
// CONEB_SWEEPS.  A block that is not finite is not iterated on.
#include "conelp_batch.hpp"
#include "batch_conelp.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == CONEB_THREADS, "the shared helpers are written for the workgroup of k_conelp_batch");
static_assert(CONEB_MAX_M * CONEB_MAX_M <= NT, "a thread per entry of a block");
static_assert(CONELP_NSTAT == CONEB_NSTAT, "the stats of conelp_member");
#include "batch_cone.hpp"

__global__ void __launch_bounds__(CONEB_THREADS) k_conelp_batch(ConelpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int ml = a.ml, nq = a.nq, ns = a.ns, Ms = a.Ms;
    const Layout L = layout(a.n, ml, Ms, a.N, a.Nd, a.Np, nq, ns, a.p);
    Member M;
    conelp_data(M, a, a.N);
    M.ml = ml; M.nq = nq; M.ns = ns; M.Ms = Ms; M.Nd = a.Nd; M.Np = a.Np; M.ldn = L.ldn; M.ldp = L.ldp;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K; M.w = lds + L.w; M.g = lds + L.g;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.x1 = lds + L.x1;
    M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry; M.y1 = lds + L.y1;
    M.s = lds + L.s; M.z = lds + L.z; M.ds = lds + L.ds; M.dz = lds + L.dz; M.rz = lds + L.rz; M.ws3 = lds + L.ws3;
    M.z1 = lds + L.z1; M.tw = lds + L.tw; M.th = lds + L.th; M.r = lds + L.r; M.rti = lds + L.rti;
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
    conelp_member(Cone{M}, a);
}

}  // namespace

size_t conelp_batch_lds_bytes(int n, int ml, int nq, const unsigned short *q, int ns, const unsigned char *m, int p)
{
    const Sizes z = sizes(ml, nq, q, ns, m);
    return (size_t)layout(n, ml, z.Ms, z.N, z.Nd, z.Np, nq, ns, p).total * sizeof(double);
}

hipError_t launch_conelp_batch(hipStream_t st, const ConelpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_conelp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_conelp_batch<<<dim3((unsigned)a.B), dim3(CONEB_THREADS), conelp_batch_lds_bytes(a.n, a.ml, a.nq, a.q, a.ns, a.m, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
