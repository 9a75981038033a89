// k_lp_batch: one workgroup (256 threads, four wavefronts) carries one small dense LP from its starting point to its status or
// its infeasibility certificate (lp_batch.hpp).  It is conelp_member (batch_conelp.hpp) on the orthant alone: the policy below is
// the orthant part of that header's protocol and nothing else, with the Newton solve of batch_kkt.hpp on S = G' diag(di^2) G.
//
// Everything a member iterates on lives in LDS: S, its factor in place, X and K (their region holds the staged rows of diag(di) G
// while S is assembled), four n-vectors (x, dx, rx, x1), four p-vectors and ten ml-vectors (s, z, d, di, lmbda, ds, dz, rz, ws3,
// z1); th = W^-T h is recomputed as di h where it is used.  c, G, h, A, b are read from HBM / L2.
#include "lp_batch.hpp"
#include "batch_conelp.hpp"

#include <cmath>

namespace kvx {
namespace {

using namespace batchdev;
static_assert(NT == LPB_THREADS, "the shared helpers are written for the workgroup of k_lp_batch");
static_assert(CONELP_NSTAT == LPB_NSTAT, "the stats of conelp_member");

struct Layout {                               // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ldn, ldp;
    int S, XK, X, K, x, dx, rx, x1, y, dy, ry, y1, s, z, d, di, lm, ds, dz, rz, ws3, z1, red, total;
};

__host__ __device__ inline Layout layout(int n, int ml, int p)
{
    Layout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(LPB_TILE * L.ldn);
    L.XK = L.X = o; L.K = o + xsz; o += (xsz + ksz > tsz ? xsz + ksz : tsz);
    const int nv = even(n), pv = even(p), mv = even(ml);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv; L.x1 = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv; L.y1 = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.d = o; o += mv; L.di = o; o += mv; L.lm = o; o += mv;
    L.ds = o; o += mv; L.dz = o; o += mv; L.rz = o; o += mv; L.ws3 = o; o += mv; L.z1 = o; o += mv;
    L.red = o; o += NW * NRED;
    L.total = o;
    return L;
}

struct Member : ConelpMem {                   // N = ml
    double *d, *di, *lm;
};

struct Orthant {                              // the cone of conelp_member
    const Member &M;

    __device__ __forceinline__ int lmbda_len() const { return M.N; }
    template <class F>
    __device__ __forceinline__ void for_rows(F f) const { plain_rows(M.N, f); }
    __device__ __forceinline__ void load_h(double *out) const
    {
        for (int k = threadIdx.x; k < M.N; k += NT) out[k] = M.h[k];
    }
    __device__ __forceinline__ void start() const
    {
        for (int k = threadIdx.x; k < M.N; k += NT) { M.d[k] = 1.0; M.di[k] = 1.0; M.s[k] = M.h[k]; M.z[k] = 0.0; }
        __syncthreads();
    }
    __device__ __forceinline__ void max_step(const double *u0, double a0, const double *u1, double a1, double (&mx)[2]) const
    {
        orth_max_step(M.N, u0, a0, u1, a1, mx);
        blk_reduce<2, true>(mx, M.red);
    }
    __device__ __forceinline__ void push(bool ps, bool pz, const double (&mx)[2]) const { orth_push(M.N, ps, pz, mx, M.s, M.z); }
    __device__ __forceinline__ bool first_scaling() const
    {
        orth_first_scaling(M.N, M.s, M.z, M.d, M.di, M.lm);
        return true;
    }
    __device__ __forceinline__ double lam_sq() const { return sum_sq(M.lm, M.N, M.red); }
    __device__ __forceinline__ void prepare() const {}
    __device__ __forceinline__ void assemble(bool sing) const
    {
        kkt_s_init(M, sing);
        for (int k0 = 0; k0 < M.N; k0 += LPB_TILE) {
            const int kt = min((int)LPB_TILE, M.N - k0);
            __syncthreads();                               // the staged rows of the previous step have been read
            orth_stage<LPB_TILE>(M, M.G, M.N, M.di, k0, kt);
            __syncthreads();
            kkt_s_add_rows(M, kt);
        }
        __syncthreads();
    }
    __device__ __forceinline__ void kkt_before(double *vx, double *vz) const { orth_kkt_before(M.G, M.N, M.n, M.di, vx, vz); }
    __device__ __forceinline__ void kkt_after(double *vx, double *vz) const { orth_kkt_after(M.G, M.N, M.n, M.di, vx, vz); }
    __device__ __forceinline__ void gemv_t(const double *u, double sign, double *v) const
    {
        gemv_t_add(M.G, M.N, M.n, u, nullptr, sign, v);
    }
    __device__ __forceinline__ void rhs(int i, double sigma, double mu) const
    {
        orth_rhs<true>(M.N, i, sigma, mu, M.lm, M.ws3, M.d, M.rz, M.ds, M.dz);
    }
    __device__ __forceinline__ double th_dot(const double *dz) const
    {
        double acc = 0.0;
        for (int k = threadIdx.x; k < M.N; k += NT) acc += M.di[k] * M.h[k] * dz[k];
        return acc;
    }
    __device__ __forceinline__ void combine(int i, double dtau, double (&mx)[2]) const
    {
        orth_combine(M.N, i, dtau, M.lm, M.z1, M.ds, M.dz, M.ws3, mx);
        blk_reduce<2, true>(mx, M.red);
    }
    __device__ __forceinline__ void update(double step) const { orth_update(M.N, step, M.ds, M.dz, M.d, M.di, M.lm, M.s, M.z); }
};

__global__ void __launch_bounds__(LPB_THREADS) k_lp_batch(LpBatchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const Layout L = layout(a.n, a.ml, a.p);
    Member M;
    conelp_data(M, a, a.ml);
    M.ldn = L.ldn; M.ldp = L.ldp;
    M.S = lds + L.S; M.T = lds + L.XK; M.X = lds + L.X; M.K = lds + L.K;
    M.x = lds + L.x; M.dx = lds + L.dx; M.rx = lds + L.rx; M.x1 = lds + L.x1;
    M.y = lds + L.y; M.dy = lds + L.dy; M.ry = lds + L.ry; M.y1 = lds + L.y1;
    M.s = lds + L.s; M.z = lds + L.z; M.d = lds + L.d; M.di = lds + L.di; M.lm = lds + L.lm; M.ds = lds + L.ds; M.dz = lds + L.dz;
    M.rz = lds + L.rz; M.ws3 = lds + L.ws3; M.z1 = lds + L.z1; M.red = lds + L.red;
    conelp_member(Orthant{M}, a);
}

}  // namespace

size_t lp_batch_lds_bytes(int n, int ml, int p) { return (size_t)layout(n, ml, p).total * sizeof(double); }

hipError_t launch_lp_batch(hipStream_t st, const LpBatchArgs &a)
{
    // per device, so asked of the current one at every launch
    const hipError_t e = hipFuncSetAttribute((const void *)k_lp_batch, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    k_lp_batch<<<dim3((unsigned)a.B), dim3(LPB_THREADS), lp_batch_lds_bytes(a.n, a.ml, a.p), st>>>(a);
    return hipGetLastError();
}

}  // namespace kvx
