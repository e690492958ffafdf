// The launch layer of the GRU backward entry points (csrc/gru_bwd.hip, csrc/gru_bwd_fused.hip), host code only: runtime flags
// to template arguments, the launch of one instantiation, the slab workspace with its reduction, and the checks of the upstream
// gradient.  An entry point reads: validate -> describe the launch -> dispatch -> reduce.
#pragma once
#include "gru_common.h"
#include <type_traits>

namespace tmpnn {

// A runtime value that is one of the listed constants (the last one stands for "anything else", as the `else` of a ladder).
// dispatch(f, OneOf<..>{a}, OneOf<..>{b}, ...) calls f(std::integral_constant<..>{}, ...) with the matching constants, which a
// generic lambda uses as template arguments: a new instantiation is one more call of launch_k in one place.
template <auto V, auto... Vs> struct OneOf { decltype(V) v; };
using Flag = OneOf<true, false>;
using UpSel = OneOf<1, 2, 3>;                  // DhSrc as the UP template argument: bit 0 d_hout, bit 1 dy (check_upstream: never 0)
inline UpSel up_sel(const float* d_hout, const float* dy) { return UpSel{(d_hout ? 1 : 0) | (dy ? 2 : 0)}; }

template <class F> void dispatch(F&& f) { f(); }
template <class F, auto V, auto... Vs, class... Rest>
void dispatch(F&& f, OneOf<V, Vs...> s, Rest... rest) {
    if constexpr (sizeof...(Vs) > 0) {
        if (s.v != V) return dispatch(f, OneOf<Vs...>{s.v}, rest...);
    }
    dispatch([&](auto... cs) { f(std::integral_constant<decltype(V), V>{}, cs...); }, rest...);
}

// one launch; dynamic LDS above the default limit is allowed once per (instantiation, device)
template <auto Kernel, class... A>
void launch_k(dim3 grid, dim3 block, size_t shm, hipStream_t st, const A&... args) {
    if (shm) TM_SHM_ONCE(*Kernel, shm);
    hipLaunchKernelGGL(Kernel, grid, block, shm, st, args...);
}

// The weight-gradient slabs of one launch at the front of a workspace: n_rs partial sums [3H][IN+H] (w) and [2][3H] (b), one per
// block or row slab.  (bytes() still reserves the fold scratch of the former two-launch reduction behind them: callers size their
// workspaces with it; the one-launch reduction keeps its group sums in LDS and leaves that room unused.)
struct GruSlabs {
    int n_rs;
    size_t nW, nB;
    float *w, *b;
    GruSlabs(void* ws, int n_rs_, int IN, int H)
        : n_rs(n_rs_), nW((size_t)3 * H * (IN + H)), nB((size_t)6 * H), w(reinterpret_cast<float*>(ws)),
          b(w + (size_t)n_rs_ * nW) {}
    static size_t bytes(int n_rs, int IN, int H) {
        const size_t per = (size_t)3 * H * (IN + H) + (size_t)6 * H;
        return ((size_t)n_rs * per + reduce_slabs_ws_floats(n_rs, per)) * sizeof(float);
    }
    // the bias slabs' two segments of a reduction: db_ih += b[0:3H], db_hh += b[3H:6H]
    void add_bias(SlabSegs& t, int H, float* db_ih, float* db_hh) const {
        t.add(b, nB, db_ih, 1, 3 * H, 0, 0, 1);
        t.add(b + 3 * H, nB, db_hh, 1, 3 * H, 0, 0, 1);
    }
};

// the slabs' ordered sums in one launch (launch_reduce_segs, csrc/agg.hip; more than 64 slabs: 32 at a time, then the groups):
// dW_ih[j][0:IN] (row stride ld_dwih) += the W_ih block of the slabs; with `full`, dW_hh, db_ih and db_hh += theirs as well
int launch_gru_reduce_w(const GruSlabs& s, int IN, int H, float* dW_ih, int ld_dwih, float* dW_hh, float* db_ih, float* db_hh,
                        int full, hipStream_t st);

// the upstream gradient as every entry point takes it (DhSrc): d_hout [.., ld_dhout] and / or dy with the head's weights
inline int check_upstream(const char* name, const float* d_hout, int ld_dhout, const float* dy, const float* w_head, int H) {
    TM_REQUIRE(d_hout != nullptr || dy != nullptr, "%s: no upstream gradient", name);
    TM_REQUIRE(dy == nullptr || (w_head != nullptr && aligned16(w_head)), "%s: dy needs a 16-byte aligned w_head", name);
    TM_REQUIRE(d_hout == nullptr || ld_dhout >= H, "%s: ld_dhout=%d is below H=%d", name, ld_dhout, H);
    return TMPNN_OK;
}

}  // namespace tmpnn
