// dispatch.h - how a launcher turns run-time values into template arguments, and sizes its grid (host side).
//
// A launcher names its kernel once, inside a generic lambda, and the helpers here call the lambda with the run-time
// values as std::integral_constant arguments (int_c, bool_c):
//     with_geometry(G, VEC, [&](auto g, auto v) { hipLaunchKernelGGL((k_x<g.value, v.value>), ...); });
// Each helper walks a closed list, so a kernel has exactly the instantiations its lists span, and returns false where
// the value is not in the list (nothing is launched).  A static local inside the lambda is one per instantiation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace tfr {

template <int V> using int_c = std::integral_constant<int, V>;
template <bool B> using bool_c = std::integral_constant<bool, B>;

// f(int_c<v>) for v among Vs
template <int... Vs, typename F>
inline bool with_one_of(int v, F&& f) {
    // (a left fold: the lambda's bodies, and the kernels they name, are instantiated in list order - a right fold's come out reversed)
    return (... || (v == Vs ? (f(int_c<Vs>{}), true) : false));
}

// f(bool_c<b>)
template <typename F>
inline void with_bool(bool b, F&& f) {
    if (b) f(bool_c<true>{});
    else f(bool_c<false>{});
}

// Row geometry: G lanes of a wave own one row, VEC consecutive floats each (G * VEC >= D).  Every kernel that is compiled
// per row width is compiled for these ten pairs.
struct RowGeometry { int G, VEC; };
constexpr RowGeometry ROW_GEOMETRIES[] = {{4, 4}, {8, 4}, {16, 4}, {32, 4}, {64, 4}, {4, 1}, {8, 1}, {16, 1}, {32, 1}, {64, 1}};
constexpr size_t N_ROW_GEOMETRIES = sizeof(ROW_GEOMETRIES) / sizeof(ROW_GEOMETRIES[0]);

constexpr bool is_row_geometry(int G, int VEC) {
    for (size_t k = 0; k < N_ROW_GEOMETRIES; ++k)
        if (ROW_GEOMETRIES[k].G == G && ROW_GEOMETRIES[k].VEC == VEC) return true;
    return false;
}

// row geometry for a dim: returns false if unsupported
constexpr bool geometry(int D, int* G, int* VEC) {
    if (D < 1) return false;
    int vec = (D % 4 == 0) ? 4 : 1;
    int lanes = (D + vec - 1) / vec;
    int g = 4;
    while (g < lanes) g <<= 1;
    if (g > 64) return false;
    *G = g; *VEC = vec;
    return true;
}

constexpr bool every_width_has_a_listed_geometry() {
    for (int D = 1; D <= 256; ++D) {
        int G = 0, VEC = 0;
        if (geometry(D, &G, &VEC) && !is_row_geometry(G, VEC)) return false;
    }
    return true;
}
static_assert(every_width_has_a_listed_geometry(), "geometry() yields a (G, VEC) that ROW_GEOMETRIES does not list: no kernel would be launched");

template <typename F, size_t... K>
inline bool with_geometry_at(int G, int VEC, F&& f, std::index_sequence<K...>) {
    return (... || ((G == ROW_GEOMETRIES[K].G && VEC == ROW_GEOMETRIES[K].VEC)
                        ? (f(int_c<ROW_GEOMETRIES[K].G>{}, int_c<ROW_GEOMETRIES[K].VEC>{}), true)
                        : false));
}
// f(int_c<G>, int_c<VEC>) for the listed pair
template <typename F>
inline bool with_geometry(int G, int VEC, F&& f) {
    return with_geometry_at(G, VEC, f, std::make_index_sequence<N_ROW_GEOMETRIES>{});
}

// blocks of a launch that gives each block per_block units of n and grid-strides past cap: ceil(n / per_block) in [1, cap]
constexpr int blocks_for(int64_t n, int64_t per_block, int64_t cap = INT32_MAX) {
    int64_t nb = (n + per_block - 1) / per_block;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    return (int)nb;
}

}  // namespace tfr
