// bayhunter_amd/csrc/bh_hostkit.h -- the host plumbing of the chain-diagnostics units (chain_diag_kernel.hip, chain_ladder_kernel.hip,
// chain_rank_kernel.hip, chain_ladder_evidence_kernel.hip; chain_ladder_sweep_kernel.hip takes fail and BH_CHK) and of the posterior
// handle (posterior_common.h): a device buffer that goes with its frame, the refusal through the engine's last error, the check of
// a HIP call, and the staging of what a call of memspace BH_HOST brings.  Header only; every function is host code around HIP calls.
// (bh_engine_impl.h's DevBuf / ensure are another thing: workspaces the engine owns and grows.)
#ifndef BH_HOSTKIT_H
#define BH_HOSTKIT_H

#include "bh_device.h"
#include "../../include/bh_engine.h"

#include <string>
#include <vector>

namespace bhkit {

struct Buf {
    void *p = nullptr;
    ~Buf() { if (p) (void)hipFree(p); }
    template <typename U> U *as() const { return (U *)p; }
};

inline int fail(bh_engine *e, int code, const std::string &what) { return bh_engine_fail_internal(e, code, what.c_str()); }

// a HIP call of a function that returns the engine's codes: its error is the function's BH_EHIP
#define BH_CHK(e, call)                                                                                             \
    do {                                                                                                            \
        hipError_t _he = (call);                                                                                    \
        if (_he != hipSuccess) return bhkit::fail((e), BH_EHIP, std::string(#call ": ") + hipGetErrorString(_he)); \
    } while (0)

// b must hold nothing
inline int alloc(bh_engine *e, Buf &b, size_t bytes)
{
    hipError_t he = hipMalloc(&b.p, bytes ? bytes : 8);
    if (he != hipSuccess) { b.p = nullptr; return fail(e, BH_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(he)); }
    return BH_OK;
}

template <typename U> int upload(bh_engine *e, hipStream_t st, Buf &b, const std::vector<U> &v)
{
    int rc;
    if ((rc = alloc(e, b, v.size() * sizeof(U)))) return rc;
    if (!v.empty()) BH_CHK(e, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice, st));
    return BH_OK;
}

// the stream of a call: the caller's with device tables (where it names one), else the engine's
inline hipStream_t call_stream(bh_engine *e, int memspace, void *stream)
{
    return (memspace == BH_DEVICE && stream) ? (hipStream_t)stream : (hipStream_t)bh_engine_stream(e);
}

// a table on the device: the caller's pointer, or (memspace BH_HOST) a copy of the `bytes` its span covers -- the span is the
// caller's to state: every table has its own
template <typename P> int stage(bh_engine *e, hipStream_t st, int memspace, const P *x, size_t bytes, Buf &copy, const P **dx)
{
    *dx = x;
    if (memspace == BH_DEVICE) return BH_OK;
    int rc;
    if ((rc = alloc(e, copy, bytes))) return rc;
    BH_CHK(e, hipMemcpyAsync(copy.p, x, bytes, hipMemcpyHostToDevice, st));
    *dx = (const P *)copy.p;
    return BH_OK;
}

} // namespace bhkit
#endif
