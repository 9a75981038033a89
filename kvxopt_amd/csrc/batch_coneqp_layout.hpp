// The LDS of one member of a cone QP as k_coneqp_batch (coneqp_batch.hip) and k_coneqp_batch_diff (coneqp_batch_diff.hip) lay it
// out.  The member has no x1, y1, z1 and no W^-T h: the layout is that of batch_cone.hpp
// without those four vectors, so it is smaller at every shape.
//
// This file is text of its includer: it is included once, after batch_cone.hpp, inside the anonymous namespace of kvx.
struct QpLayout {                             // offsets in doubles from the LDS base; every part starts on 16 bytes
    int ldn, ldp;
    int S, XK, X, K, w, g, x, dx, rx, y, dy, ry, s, z, ds, dz, rz, ws3, tw, r, rti, lm, d, di, beta, sgs, sgz, wk, nrm, red, off, blk,
        cone, prow, pmir, flag, total;
};

// Ms: the first 's' row, ml + sum q_k.  The parts are those of layout() of batch_cone.hpp without x1, y1, z1 and th.
__host__ __device__ inline QpLayout qp_layout(int n, int ml, int Ms, int N, int Nd, int Np, int nq, int ns, int p)
{
    QpLayout L;
    L.ldn = n | 1;
    L.ldp = p | 1;
    int o = 0;
    L.S = o; o += even(n * L.ldn);
    const int xsz = even(p * L.ldn), ksz = even(p * L.ldp), tsz = even(CONEB_TILE * L.ldn), wsz = ns ? even(CONEB_MAX_M * L.ldn) : 0,
              gsz = nq ? even(RING * L.ldn) : 0;
    L.XK = L.X = o; L.K = o + xsz; L.w = o + tsz; L.g = o + tsz + wsz;
    o += (xsz + ksz > tsz + wsz + gsz ? xsz + ksz : tsz + wsz + gsz);
    const int nv = even(n), pv = even(p), mv = even(N), sv = even(N - Ms), lv = even(ml), cv = even(Ms), dv = even(Nd), ev = even(Nd - Ms);
    L.x = o; o += nv; L.dx = o; o += nv; L.rx = o; o += nv;
    L.y = o; o += pv; L.dy = o; o += pv; L.ry = o; o += pv;
    L.s = o; o += mv; L.z = o; o += mv; L.ds = o; o += mv; L.dz = o; o += mv; L.rz = o; o += mv; L.ws3 = o; o += mv; L.tw = o; o += mv;
    L.r = o; o += sv; L.rti = o; o += sv;
    L.lm = o; o += dv; L.d = o; o += cv; L.di = o; o += lv; L.beta = o; o += even(nq); L.sgs = o; o += ev; L.sgz = o; o += ev;
    L.wk = o; o += ns ? 4 * MM : 0;
    L.nrm = o; o += ns ? 2 * CONEB_MAX_M : 0;
    L.red = o; o += NW * NRED;
    L.off = o; o += even((nq + 2) / 2);                    // nq + 1 ints
    L.blk = o; o += even(ns + 1);                          // 2 (ns + 1) ints
    L.cone = o; o += even((Ms - ml + 3) / 4);              // sum q_k unsigned shorts
    L.prow = o; o += even((Np + 3) / 4);                   // Np unsigned shorts
    L.pmir = o; o += even((Np + 3) / 4);
    L.flag = o; o += 2;
    L.total = o;
    return L;
}
