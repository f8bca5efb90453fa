// Stand-alone check of the host-side argument validation of dm_jbu_apply_bwd_filters_f32 and dm_jbu_apply_bwd_source_f32, meant to be built
// with the host sanitizers and run on the CPU: every call below must return DM_EINVAL, with a message, BEFORE anything touches a
// device (no GPU is needed, none is used).  Nothing sanitized is loaded into Python.
//
//   cd densematcher_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I ../../include -I . -Xarch_host -fsanitize=address,undefined \
//         ../../tools/jbu_bwd_args_check.hip dm_jbu_bwd.hip dm_ctx.hip -o ../build/jbu_bwd_args_check && ../build/jbu_bwd_args_check
#include <stdio.h>
#include <string.h>

#include "dm_internal.h"

static int failures = 0;

static void expect_einval(dm_ctx* ctx, const char* what, int rc) {
    const char* msg = dm_last_error(ctx);
    const bool ok = rc == DM_EINVAL && (!ctx || (msg && strlen(msg) > 0));
    printf("%-44s rc %d %s\n", what, rc, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
    if (ctx) ctx->err.clear();
}

int main() {
    dm_ctx ctx;                       // never given a device: a call that got past its checks would fail in hipSetDevice, not here
    static float buf[16];
    const long long S[4] = {64, 16, 4, 1};
    void* src = buf;
    float* f = buf;
#define FILTERS(B, C, h, w, dt, s, s2, g, g2, out) \
    dm_jbu_apply_bwd_filters_f32(&ctx, B, C, h, w, dt, s, S[0], S[1], s2, S[3], g, S[0], S[1], g2, S[3], out)
#define SOURCE(B, C, h, w, g, g2, fl, out) dm_jbu_apply_bwd_source_f32(&ctx, B, C, h, w, g, S[0], S[1], g2, S[3], fl, out)
    expect_einval(nullptr, "filters: null context", dm_jbu_apply_bwd_filters_f32(nullptr, 1, 1, 2, 2, DM_F32, src, 0, 0, 0, 0, f, 0, 0, 0, 0, f));
    expect_einval(&ctx, "filters: B = 0", FILTERS(0, 1, 2, 2, DM_F32, src, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: B = 65536", FILTERS(65536, 1, 2, 2, DM_F32, src, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: C = 0", FILTERS(1, 0, 2, 2, DM_F32, src, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: h = 1", FILTERS(1, 1, 1, 2, DM_F32, src, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: w = 0", FILTERS(1, 1, 2, 0, DM_F32, src, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: h = 8193", FILTERS(1, 1, 8193, 2, DM_F32, src, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: unknown dtype", FILTERS(1, 1, 2, 2, 7, src, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: null source", FILTERS(1, 1, 2, 2, DM_F32, nullptr, S[2], f, S[2], f));
    expect_einval(&ctx, "filters: null gout", FILTERS(1, 1, 2, 2, DM_F32, src, S[2], nullptr, S[2], f));
    expect_einval(&ctx, "filters: null gfilt", FILTERS(1, 1, 2, 2, DM_F32, src, S[2], f, S[2], nullptr));
    expect_einval(&ctx, "filters: negative source stride", FILTERS(1, 1, 2, 2, DM_F16, src, -4, f, S[2], f));
    expect_einval(&ctx, "filters: negative gout stride", FILTERS(1, 1, 2, 2, DM_F32, src, S[2], f, -4, f));
    expect_einval(nullptr, "source: null context", dm_jbu_apply_bwd_source_f32(nullptr, 1, 1, 2, 2, f, 0, 0, 0, 0, f, f));
    expect_einval(&ctx, "source: B = 0", SOURCE(0, 1, 2, 2, f, S[2], f, f));
    expect_einval(&ctx, "source: C = -1", SOURCE(1, -1, 2, 2, f, S[2], f, f));
    expect_einval(&ctx, "source: h = 0", SOURCE(1, 1, 0, 2, f, S[2], f, f));
    expect_einval(&ctx, "source: w = 1", SOURCE(1, 1, 2, 1, f, S[2], f, f));
    expect_einval(&ctx, "source: w = 8193", SOURCE(1, 1, 2, 8193, f, S[2], f, f));
    expect_einval(&ctx, "source: null gout", SOURCE(1, 1, 2, 2, nullptr, S[2], f, f));
    expect_einval(&ctx, "source: null filters", SOURCE(1, 1, 2, 2, f, S[2], nullptr, f));
    expect_einval(&ctx, "source: null gsrc", SOURCE(1, 1, 2, 2, f, S[2], f, nullptr));
    expect_einval(&ctx, "source: negative gout stride", SOURCE(1, 1, 2, 2, f, -4, f, f));
    printf(failures ? "%d FAILED\n" : "all refused before any launch\n", failures);
    return failures ? 1 : 0;
}
