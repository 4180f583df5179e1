// host_util.h — the host-side helpers every module's extern "C" section shares (internal, host only; include after
// gdr_common.h).  The error text of a call is set_error's (api.hip); these pair it with the status the entry point returns.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gdr {

static inline int invalid_arg(const char* what) {
    set_error(what, hipSuccess);
    return GDR_ERR_INVALID_ARG;
}

// the status of the launches an entry point has just issued; `what` names the kernel
static inline int launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return GDR_OK;
    set_error(what, e);
    return GDR_ERR_HIP;
}

static inline int unsupported(const char* what) {
    set_error(what, hipSuccess);
    return GDR_ERR_UNSUPPORTED;
}

static inline int workspace_too_small(const char* what) {
    set_error(what, hipSuccess);
    return GDR_ERR_WORKSPACE;
}

static inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// mask = alignment in bytes - 1; a NULL pointer is aligned
static inline bool misaligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }

// a storage type code (GDR_F16 / GDR_BF16 / GDR_F32)
static inline bool bad_dtype(int32_t dt) { return dt < GDR_F16 || dt > GDR_F32; }
static inline size_t esize(int32_t dt) { return dt == GDR_F32 ? 4 : 2; }      // the bytes of one element

// a (rows, C) matrix read or written in 8-element pieces: 16-byte base, a stride that is a multiple of 8 and at least C
static inline bool bad_rows(const void* ptr, int64_t stride, int64_t C) { return misaligned(ptr, 15) || stride < C || stride % 8; }

// the slabs a partial sum over n rows is cut into: one per slab_min rows, max_slabs at most
static inline int slabs_of(int64_t n, int slab_min, int max_slabs) {
    const int64_t s = (n + slab_min - 1) / slab_min;
    return s < 1 ? 1 : (s > max_slabs ? max_slabs : (int)s);
}

}  // namespace gdr
