// What the host entries of the batch solvers share (qp_batch_api.cpp, lp_batch_api.cpp): the refusal with its message, the
// question for a device, and the device copies of one host call.
#pragma once
#include "../../include/kvxhip.h"
#include "abi_guard.hpp"
#include "devpool.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#define HIPCHK(call)                                                             \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return KVX_EDEVICE;                                \
    } while (0)

namespace kvx {
namespace batchhost {

inline int refuse(const char *who, const std::string &why)
{
    set_last_error(std::string(who) + ": " + why);
    return KVX_EINVAL;
}

inline int need_device(const char *who)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) {
        set_last_error(std::string(who) + ": no HIP device; the batch has no CPU fallback");
        return KVX_EDEVICE;
    }
    return KVX_OK;
}

struct Buffers {                              // the device copies of one host call, given back to the pool on every path
    std::vector<void *> own;
    ~Buffers() { for (void *p : own) (void)pool_free(p); }
    int get(double **d, int64_t count)
    {
        HIPCHK(pool_malloc((void **)d, (size_t)(count > 0 ? count : 1) * sizeof(double)));
        own.push_back(*d);
        return KVX_OK;
    }
    int up(const double **d, const double *h, int64_t count)
    {
        double *t = nullptr;
        int rc = get(&t, count);
        if (rc) return rc;
        if (count > 0) HIPCHK(hipMemcpy(t, h, (size_t)count * sizeof(double), hipMemcpyHostToDevice));
        *d = t;
        return KVX_OK;
    }
};

inline int down(void *h, const void *d, int64_t count)
{
    if (count > 0) HIPCHK(hipMemcpy(h, d, (size_t)count * 8, hipMemcpyDeviceToHost));
    return KVX_OK;
}

}  // namespace batchhost
}  // namespace kvx
