// Host-only helpers for the device arenas of the handles: one rounding rule, one carver, and one name for the four weight
// matrices of a DiT block.  No device code here.
#pragma once
#include <stddef.h>

#include "t2s_common.h"

namespace t2s {

// every piece of an arena starts on a multiple of 64 elements (256 B of fp32)
inline size_t r64(size_t n) { return (n + 63) & ~size_t(63); }

// Hands out consecutive pieces of ONE device allocation of T, each rounded up to 64 elements, to pointer slots of any
// element type (n counts T).  A layout is written once, as a function that calls take(slot, n) for every piece in order;
// it runs with a null base to measure (off = the total, no slot touched) and with the allocation to bind.
template <class T>
struct Carver {
    T* base = nullptr;
    size_t off = 0;
    template <class P>
    void operator()(P*& slot, size_t n) {
        if (base) slot = reinterpret_cast<P*>(base + off);
        off += r64(n);
    }
};

// measure `layout`, allocate it, bind it.  On failure nothing is bound and arena stays NULL; *elems = the size asked for
template <class T, class L>
hipError_t carve_alloc(T*& arena, L&& layout, size_t* elems = nullptr) {
    Carver<T> measure;
    layout(measure);
    if (elems) *elems = measure.off;
    arena = nullptr;
    const hipError_t e = hipMalloc(&arena, measure.off * sizeof(T));
    if (e != hipSuccess) {
        arena = nullptr;
        return e;
    }
    Carver<T> bind{arena};
    layout(bind);
    return hipSuccess;
}

// The four weight matrices of a DiT block, W (N, K) row-major: one set per form they are kept in (packed fp32 for the 32- and
// the 16-token row kernels, bf16 planes, the training packs of W and W^T, their biases)
enum { QKV = 0, PROJ = 1, FC1 = 2, FC2 = 3, NMAT = 4 };
constexpr int MAT_N[NMAT] = {3 * D, D, 2 * D, D}, MAT_K[NMAT] = {D, D, D, 2 * D};
constexpr size_t mat_elems(int j) { return (size_t)MAT_N[j] * MAT_K[j]; }
template <class P>
struct BlockMats {
    P m[NMAT];
    P& operator[](int j) { return m[j]; }
    const P& operator[](int j) const { return m[j]; }
};
// matrix j / its bias in t2s_dit_block_weights and t2s_dit_block_grads (declared qkv_w, qkv_b, proj_w, ... fc2_b, ada_w, ada_b)
template <class B>
auto mat_w(const B& b, int j) { return (&b.qkv_w)[2 * j]; }
template <class B>
auto mat_b(const B& b, int j) { return (&b.qkv_w)[2 * j + 1]; }
static_assert(offsetof(t2s_dit_block_weights, fc2_b) == 7 * sizeof(void*) && offsetof(t2s_dit_block_grads, fc2_b) == 7 * sizeof(void*),
              "mat_w / mat_b index the block structs as pointer arrays");

}  // namespace t2s
