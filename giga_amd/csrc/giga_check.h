// Host-side argument checks that the extern "C" entry points of more than one file share.  Host code only.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/giga_hip.h"

namespace giga {

// offsets of a ragged batch (host array of B + 1 entries): starts at 0 and never decreases
inline bool ragged_ok(const int32_t* offs, int B) {
    if (!offs || offs[0] != 0) return false;
    for (int b = 0; b < B; ++b)
        if (offs[b + 1] < offs[b]) return false;
    return true;
}
inline int ragged_batch_check(int B) { return B < 0 ? -1 : (B > GIGA_MAX_SCENES ? -7 : 0); }

// the largest item of a ragged batch (offsets that ragged_ok accepted)
inline int ragged_max_count(const int32_t* offs, int B) {
    int m = 0;
    for (int b = 0; b < B; ++b) m = offs[b + 1] - offs[b] > m ? offs[b + 1] - offs[b] : m;
    return m;
}

// a ragged batch of B meshes: both offset arrays are well formed, and data that is not empty has a pointer
inline bool mesh_batch_check(const int32_t* vertex_offsets, const int32_t* triangle_offsets, int B, const void* vertices,
                             const void* triangles) {
    if (!ragged_ok(vertex_offsets, B) || !ragged_ok(triangle_offsets, B)) return false;
    return (vertex_offsets[B] == 0 || vertices) && (triangle_offsets[B] == 0 || triangles);
}

inline bool finite_f64(double x) { return x - x == 0.0; }

// n cameras (extrinsics [n][16], intrinsics [n][4] = fx, fy, cx, cy): every number finite, no focal length zero
inline bool camera_check(int n, const double* extrinsics, const double* intrinsics) {
    if (n > 0 && (!extrinsics || !intrinsics)) return false;
    for (size_t i = 0; i < (size_t)n * 16; ++i)
        if (!finite_f64(extrinsics[i])) return false;
    for (size_t i = 0; i < (size_t)n * 4; ++i)
        if (!finite_f64(intrinsics[i])) return false;
    for (int v = 0; v < n; ++v)
        if (intrinsics[4 * (size_t)v] == 0.0 || intrinsics[4 * (size_t)v + 1] == 0.0) return false;
    return true;
}

}  // namespace giga
