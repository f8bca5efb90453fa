// Host-side checks that every DiffusionNet translation unit makes (dm_dnet.hip, dm_dnet_layers.hip, dm_dnet_half.hip and the two
// backward files): one copy each.
#pragma once

#include "dm_internal.h"

// n_verts lives on the device and bounds every load: read it back once and refuse counts outside [1, N]
static inline int dm_dnet_check_counts(dm_ctx* ctx, const char* who, int B, int N, const int32_t* n_verts) {
    if (!n_verts) return DM_OK;
    std::vector<int32_t> h((size_t)B);
    DM_CHECK_HIP(ctx, hipMemcpyAsync(h.data(), n_verts, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    DM_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < B; ++b)
        if (h[b] < 1 || h[b] > N) return dm_fail(ctx, DM_EINVAL, "%s: n_verts[%d] = %d outside [1, %d]", who, b, (int)h[b], N);
    return DM_OK;
}

static inline bool dm_dnet_dtype(int d) { return d == DM_F16 || d == DM_F32; }
// is p a multiple of `bytes` (a power of two)?  True for a null pointer.
static inline bool dm_dnet_al(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }
