// The embedding CNN in eval mode: the entry points (tmpnn_espnet_arena_floats, tmpnn_espnet_ws_bytes, tmpnn_espnet_fwd, and for
// single pixels tmpnn_espnet_centres_ws_bytes, tmpnn_espnet_trunk, tmpnn_espnet_centres; include/tmpnn.h).  The kernels, the
// arena, the workspace and the launch sequences are espnet_net.h, which espnet_train.hip shares.
#include "espnet_net.h"

extern "C" size_t tmpnn_espnet_arena_floats(int C) {
    if (C < 1 || C > ESP_MAX_C) return 0;
    Net n;
    return walk_arena(nullptr, C, n);
}

extern "C" size_t tmpnn_espnet_ws_bytes(int T, int H, int W, int C) {
    if (!shape_ok(T, H, W, C)) return 0;
    Ws s;
    return walk_ws(nullptr, T, H, W, C, s);
}

extern "C" size_t tmpnn_espnet_centres_ws_bytes(int T, int H, int W, int C) {
    if (!shape_ok(T, H, W, C)) return 0;
    Ws s;
    return walk_ws(nullptr, T, H, W, C, s, false);
}

extern "C" int tmpnn_espnet_fwd(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes, float* out,
                                tmpnn_stream stream) {
    if (int rc = check_call("espnet_fwd", arena, images, ws, out, T, H, W, C)) return rc;
    Net n;
    walk_arena(arena, C, n);
    Ws s;
    const size_t need = walk_ws(ws, T, H, W, C, s);
    if (ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "espnet_fwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if (int rc = run_trunk(n, s, images, T, H, W, C, as_stream(stream))) return rc;
    return run_tail(n, s, T, H, W, C, out, as_stream(stream));
}

extern "C" int tmpnn_espnet_trunk(const float* arena, int C, const float* images, int T, int H, int W, void* ws, size_t ws_bytes,
                                  tmpnn_stream stream) {
    if (int rc = check_call("espnet_trunk", arena, images, ws, ws, T, H, W, C)) return rc;
    Net n;
    walk_arena(arena, C, n);
    Ws s;
    const size_t need = walk_ws(ws, T, H, W, C, s, false);
    if (ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "espnet_trunk: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return run_trunk(n, s, images, T, H, W, C, as_stream(stream));
}

extern "C" int tmpnn_espnet_centres(const float* arena, int C, int T, int H, int W, const void* ws, size_t ws_bytes, const int32_t* pix,
                                    int D, float* logits, int32_t* flags, tmpnn_stream stream) {
    TM_REQUIRE(D >= 0, "espnet_centres: D=%d", D);
    TM_REQUIRE(arena != nullptr && ws != nullptr && (D == 0 || (pix != nullptr && logits != nullptr && flags != nullptr)),
               "espnet_centres: null pointer (arena, ws, pix, logits, flags)");
    TM_REQUIRE(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "espnet_centres: H=%d W=%d (positive multiples of 16)", H, W);
    TM_REQUIRE(shape_ok(T, H, W, C) && (int64_t)T * H * W < ((int64_t)1 << 31), "espnet_centres: T=%d C=%d H=%d W=%d (a shape "
               "tmpnn_espnet_trunk takes, T H W < 2^31)", T, C, H, W);
    TM_REQUIRE(C <= ESPC_MAX_C, "espnet_centres: C=%d (1 .. %d; wider nets take the dense call, tmpnn_espnet_fwd)", C, ESPC_MAX_C);
    TM_REQUIRE(aligned16(arena) && aligned16(ws), "espnet_centres: arena and ws must be 16-byte aligned");
    Net n;
    walk_arena(arena, C, n);
    Ws s;
    const size_t need = walk_ws(const_cast<void*>(ws), T, H, W, C, s, false);
    if (ws_bytes < need) return set_error(TMPNN_EWORKSPACE, "espnet_centres: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if (D == 0) return TMPNN_OK;
    const EspTail a{s.l1, s.l2, s.m3, n.proj2.wt, n.proj2.scale, n.proj2.shift, n.proj2.slope,
                    n.proj1.wt, n.proj1.scale, n.proj1.shift, n.proj1.slope};
    k_esp_centres<<<dim3((unsigned)D), ESP_THREADS, 0, as_stream(stream)>>>(a, C, T, H, W, pix, logits, flags);
    return check_launch("espnet_centres");
}
