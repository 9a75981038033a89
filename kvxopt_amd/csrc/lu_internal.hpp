// Internal (library-private) view of the sparse LU objects shared by lu_api.cpp, lu_setup.cpp, lu_factor.cpp and lu_solve.cpp.
#pragma once
#include "../../include/kvxhip.h"
#include "abi_guard.hpp"
#include "devpool.hpp"
#include "lu_device.hpp"
#include "lu_symbolic.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

using namespace kvx;

#define HIPCHK(call)                                                             \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) {                                                  \
            set_last_error(std::string(#call) + ": " + hipGetErrorString(e_));  \
            return KVX_EDEVICE;                                                  \
        }                                                                        \
    } while (0)

struct kvx_lu_sym {
    LuSymbolic Y;
};

// Every environment knob of the LU host path.  read_lu_knobs() fills the table ONCE PER NUMERIC OBJECT, when it is created: a process
// may change a knob between two factors, never under one that exists.  KVX_LU_NO_BTF belongs to the analysis (lu_symbolic.cpp, one
// read per analysis).  DESIGN.md has the table.
struct LuKnobs {
    bool graph = true;          // KVX_LU_GRAPH=0: every call enqueues its launches itself
    bool unblocked = false;     // KVX_LU_UNBLOCKED (any value): big fronts by one workgroup each (debugging aid)
    bool lds_legacy = false;    // KVX_LU_LDS_LEGACY (any value): the LDS-resident elimination for the LDS fronts (debugging aid)
    bool wp = true;             // KVX_LU_WP=0: the round-3 kernel (two barriers per pivot) for every launch of LDS fronts
    int wp_maxcnt = 512;        // KVX_LU_WP_MAXCNT: largest launch (fronts) that k_lu_front_wp takes
    bool timing = false;        // KVX_LU_TIMING (any value): wall time of the phases of a numeric factorisation on stderr
    bool dump_plan = false;     // KVX_LU_DUMP_PLAN (any value): the levels of every plan this factor uploads on stderr
};
LuKnobs read_lu_knobs();

// The kernel of one launch of LDS fronts.  k_lu_front_wp wins where a launch is a level's few dozen fronts (its time is that of its
// slowest front); thousands of fronts per launch are bound by how many workgroups a CU holds, and the tiled kernel is the smaller
// one.  The wp kernel's work items hold 32-bit offsets into the arena.
inline LuFrontKernel lu_front_kernel(const LuKnobs &K, int count, int64_t arena_size)
{
    if (K.lds_legacy) return LU_FRONT_LEGACY;
    return K.wp && count <= K.wp_maxcnt && arena_size < (int64_t)1 << 32 ? LU_FRONT_WP : LU_FRONT_TILED;
}

struct LuLap {                                      // KVX_LU_TIMING: wall time of the phases of a numeric factorisation on stderr
    bool on;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "  lu %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// hipMalloc costs 0.1-0.7 ms on MI355X and a numeric object owns ~30 arrays: on a new pattern (nothing of the right size cached in
// the pool) that was most of a first klu.linsolve call.  The arrays of one (re)build share ONE device block and ONE host-to-device
// copy: uploads first (packed into a staging buffer in the same layout), then the uninitialised ones, every slot 256-byte aligned.
struct Arena {
    std::vector<void **> dst;
    std::vector<size_t> off, bytes;
    std::vector<const void *> src;
    size_t total = 0, upload_end = 0;
    void add(void **p, size_t b, const void *s)
    {
        dst.push_back(p); off.push_back(total); bytes.push_back(b); src.push_back(s);
        total += (std::max<size_t>(b, 1) + 255) & ~(size_t)255;
        if (s) upload_end = total;
    }
    template <class T> void up(T **p, const std::vector<T> &v) { add((void **)p, v.size() * sizeof(T), v.empty() ? (const void *)&total : (const void *)v.data()); }
    template <class T> void alloc(T **p, int64_t count) { add((void **)p, (size_t)std::max<int64_t>(count, 1) * sizeof(T), nullptr); }
    int commit(void **base)
    {
        HIPCHK(pool_malloc(base, std::max<size_t>(total, 256)));
        std::vector<char> stage(upload_end, 0);
        for (size_t i = 0; i < dst.size(); i++) {
            *dst[i] = (char *)*base + off[i];
            if (src[i] && bytes[i]) memcpy(stage.data() + off[i], src[i], bytes[i]);
        }
        if (upload_end) HIPCHK(hipMemcpy(*base, stage.data(), upload_end, hipMemcpyHostToDevice));
        return KVX_OK;
    }
};

// Device storage, one struct of typed pointers per pooled block; a block is given back by lu_free_block (pool_free + `= {}`).
struct LuStructD {              // the plan's arrays + factor storage: rebuilt with every plan (upload_structure)
    void *block = nullptr;
    LuFrontD *fr = nullptr;
    int32_t *rowidx = nullptr, *rel = nullptr, *children = nullptr, *adst = nullptr, *lists = nullptr, *slists = nullptr;
    int32_t *ipiv = nullptr, *lperm = nullptr, *fail = nullptr;
    int32_t *fcol = nullptr, *frow = nullptr, *flevpos = nullptr;          // block triangular form: F by rows / by columns
    int64_t *fptr_r = nullptr, *fptr_c = nullptr, *fsrc_r = nullptr, *fsrc_c = nullptr;
    double *fval_r = nullptr, *fval_c = nullptr;
    int64_t *asrc = nullptr, *prow = nullptr, *qcol = nullptr;
    double *Lx = nullptr, *Ux = nullptr, *arena = nullptr;
};
struct LuMatrixD {              // per-matrix arrays: once per numeric object (ensure_device)
    void *block = nullptr;
    int32_t *ai32 = nullptr;
    double *rinv = nullptr, *rmax = nullptr, *Ax = nullptr;
};
struct LuRowMapD {              // row-wise maps of the refined solve: at the first refined solve (ensure_refine)
    void *block = nullptr;
    int64_t *ap = nullptr, *csrp = nullptr;                       // column pointers of A (the rows of A'), row pointers of A
    int32_t *csrc = nullptr, *csrs = nullptr;                     // columns of the rows of A, their index in the caller's value order
};
struct LuRefineD {              // work vectors of the refined solve, for `cap` right-hand sides
    void *block = nullptr;
    double *rx = nullptr, *rd[2] = {nullptr, nullptr}, *ratio = nullptr, *part = nullptr;   // x; residual / correction (by step parity)
    double *om[2] = {nullptr, nullptr}, *omc = nullptr, *berr = nullptr;                     // omega (by step parity), the candidate's, [before, after] pairs
    int32_t *act[2] = {nullptr, nullptr};                         // per column: still improving (by step parity)
    int64_t cap = 0;
};
struct LuRhsD {                 // right-hand-side buffers (a pooled block each), for `cap` right-hand sides
    double *W = nullptr, *X = nullptr, *B = nullptr;
    int64_t cap = 0;
};
template <class Block> void lu_free_block(Block &b)
{
    if (b.block) (void)pool_free(b.block);
    b = {};
}

// Launch graphs of the steady state (klu.c:296-308: refactorisation on the recorded pivot sequence, then solves): the launches of
// a pass / of a solve captured once per key and replayed.  `version` changes with everything a captured sequence depends on
// besides the caller's buffers: the plan (front merges), the work buffers.
struct LuGraphKey {
    const void *ptr = nullptr;
    int64_t a = 0, b = 0;
    uint64_t version = 0;
    bool operator==(const LuGraphKey &o) const { return ptr == o.ptr && a == o.a && b == o.b && version == o.version; }
};
struct LuGraph {
    hipGraphExec_t exec = nullptr;
    LuGraphKey key, seen;                                         // of `exec` / of the previous call (a sequence is captured when a key comes twice in a row)
    void drop() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; }
};

struct LuLevelEvents { hipEvent_t A, B, C, D; };                  // st / st2 done with the level; fork to / join from st3

struct kvx_lu_num {
    kvx_lu_sym *sym = nullptr;
    LuKnobs K;                                                    // the environment knobs as they stood when this object was created
    LuPlan P;
    int64_t n = 0, nnz = 0;
    bool dev = false, factored = false;
    hipStream_t st = nullptr, st2 = nullptr, st3 = nullptr;   // st2: the blocked big-front chain of a level runs beside its LDS fronts;
                                                              // st3: every other size class of a wide level
    std::vector<LuLevelEvents> ev;
    hipEvent_t ev0 = nullptr;
    LuStructD S;
    LuMatrixD M;
    LuRhsD R;
    LuDev D;                                                      // what the kernels take: filled at every plan upload
    double tol = 1e-3, stol = 1e-3;
    int64_t attempts = 0;
    // per level: does any big front of the level interchange rows in pivot block `step` of the level's schedule?  Read from the
    // recorded pivot sequence after a factorisation; a refactorisation (same sequence) leaves out the interchange launch of every
    // block that has none
    std::vector<std::vector<uint8_t>> swap_steps;
    LuGraph g_pass, g_solve[2], g_refine[2];
    uint64_t version = 1, swap_version = 0;                   // (swap_version: the interchange flags -- the passes depend on them, the solves do not)
    bool graphs_on = true;                                    // K.graph until a capture fails
    int64_t graph_replays = 0;
    // Refined solves (kvx_lu_solve_refine, lu_refine.hip).  The residual needs the caller's unscaled A: M.Ax -- the block the host
    // entry points upload the values into anyway -- is this factor's own copy; the device entry points refresh it when the analysis
    // carries KVX_LU_FLAG_KEEP_VALUES.  Everything else is allocated at the first refined solve, never for a plain one.
    bool have_vals = false;                                       // M.Ax holds the values of the current factorisation
    LuRowMapD RM;
    LuRefineD RF;
};

// lu_setup.cpp
int ensure_device(kvx_lu_num *N);                    // streams, per-matrix arrays, first plan
int upload_structure(kvx_lu_num *N);                 // (re)build the plan from the symbolic object's merge state and upload it
void free_structure(kvx_lu_num *N);
int ensure_rhs(kvx_lu_num *N, int64_t nrhs);
int ensure_refine(kvx_lu_num *N, int64_t nrhs);
int lu_wait_for_caller(kvx_lu_num *N);
// lu_factor.cpp
int run_graphed(kvx_lu_num *N, LuGraph &g, LuGraphKey key, const std::function<int()> &body);
int factor_loop(kvx_lu_num *N, const double *Ax_dev, int reuse);
// lu_solve.cpp: every solve entry point.  steps == 0 && !berr_out is the plain solve; host: B is host memory, staged through R.B
int lu_solve_any(kvx_lu_num *N, bool host, int trans, double *B, int64_t nrhs, int64_t ldB, int64_t steps, double *berr_out);
