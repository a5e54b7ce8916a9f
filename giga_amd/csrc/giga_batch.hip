// Training batches from a device-resident training set: the draws of an item (giga_batch_draw) and the assembly of a batch from
// draws (giga_batch_assemble).  The semantics are spelled out in include/giga_hip.h; tests/resident_emu.py restates them.
//
//   draw      one launch, one lane per (item, m): every lane redoes the item's block of stream 0 (a Philox block is ~60 integer
//             instructions) and looks up its file's size, then evaluates its own index -- mulhi of a stream-1 word, or the keyed
//             Feistel bijection with cycle walking (bounded: batch_permute).  Lane m = 0 writes the item's scalars.
//   assemble  one launch, memory bound (a batch of 32 at M = 2048 moves ~8 MB each way).  The first B x GRID_BLOCKS workgroups copy
//             the grids: a lane owns four consecutive k of one output row (i, j, .); the quarter turn only permutes i and j, so
//             both sides are contiguous in k.  The store is 16 bytes; the z shift leaves the source unaligned, so it is read with
//             dword loads (the un-augmented copy reads 16 bytes too).  The remaining workgroups gather the occupancy points, one
//             lane per (item, m); lane m = 0 of an item computes its pose.
// Every double operation is one IEEE rounding: the file is compiled without contraction, so no operation needs __dmul_rn /
// __dadd_rn to hold it; the float32 divisions use __fdiv_rn.  No atomics: equal input gives equal bytes.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_philox.h"
#include <cmath>
#include <cstdint>

#include "../../include/giga_hip.h"

#pragma clang fp contract(off)

namespace giga {

constexpr int BATCH_BLOCK = 256;
constexpr int BATCH_RES = GIGA_BATCH_RES;
constexpr int BATCH_VOX = BATCH_RES * BATCH_RES * BATCH_RES;
constexpr int BATCH_ROW4 = BATCH_RES / 4;                    // 16-byte pieces of a row
constexpr int BATCH_VOX4 = BATCH_VOX / 4;
constexpr int BATCH_GRID_BLOCKS = (BATCH_VOX4 + BATCH_BLOCK - 1) / BATCH_BLOCK;
enum { BATCH_STREAM_ITEM = 0, BATCH_STREAM_OCC = 1 };

struct BatchFile { long long first; unsigned n; int scene; bool ok; };

__device__ __forceinline__ unsigned batch_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

// the scene of a row and its file range; ok = false for a row outside the table or offsets that do not fit the set
__device__ __forceinline__ bool batch_scene(const GigaBatchSet& s, int row, int& scene, int& f0, int& nf) {
    if (row < 0 || row >= s.n_rows) return false;
    scene = s.row_scene[row];
    if (scene < 0 || scene >= s.n_scenes) return false;
    f0 = s.scene_files[scene];
    const int f1 = s.scene_files[scene + 1];
    nf = f1 - f0;
    return f0 >= 0 && f1 <= s.n_files && nf > 0;
}

// the point range of file `file` of a scene's nf files starting at f0
__device__ __forceinline__ bool batch_file(const GigaBatchSet& s, int f0, int nf, int file, long long& first, unsigned& n) {
    if (file < 0 || file >= nf) return false;
    first = s.file_points[f0 + file];
    const long long count = s.file_points[f0 + file + 1] - first;
    if (first < 0 || count < 0 || count >= (1LL << 31) || first + count > s.n_points) return false;
    n = (unsigned)count;
    return true;
}

__device__ __forceinline__ unsigned batch_fmix32(unsigned h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// pi(m), m < n, 2 <= n < 2^31: the Feistel network of the header on b bits, applied again while the value is >= n.  The network is
// a bijection of [0, 2^b) and m < n, so the walk passes through at most 2^b - n values >= n before it is back below n.
__device__ unsigned batch_permute(unsigned m, unsigned n, const Philox& key) {
    int b = 32 - __clz((int)(n - 1u));
    b = b < 2 ? 2 : (b + 1) & ~1;
    const int h = b >> 1;
    const unsigned mask = (1u << h) - 1u;
    const unsigned long long outside = (1ull << b) - (unsigned long long)n;
    unsigned v = m;
    for (unsigned long long it = 0; it <= outside; ++it) {
        unsigned L = v >> h, R = v & mask;
#pragma unroll
        for (unsigned r = 0; r < GIGA_BATCH_FEISTEL_ROUNDS; ++r) {
            const unsigned t = L ^ (batch_fmix32(R ^ (key.x[r & 3u] + r * 0x9E3779B9u)) & mask);
            L = R;
            R = t;
        }
        v = (L << h) | R;
        if (v < n) break;
    }
    return v < n ? v : m;                     // (v < n always: see above)
}

__global__ __launch_bounds__(BATCH_BLOCK) void batch_draw_kernel(GigaBatchSet s, const int* __restrict__ ordinals, const int* __restrict__ rows,
                                                                 int M, unsigned epoch, unsigned k0, unsigned k1, int* __restrict__ quarter,
                                                                 double* __restrict__ u, int* __restrict__ file, int* __restrict__ index) {
    const int item = blockIdx.y;
    const int m = blockIdx.x * BATCH_BLOCK + threadIdx.x;
    if (m >= M && m != 0) return;
    const unsigned ordinal = (unsigned)ordinals[item];
    int scene = 0, f0 = 0, nf = 0;
    const bool ok = batch_scene(s, rows[item], scene, f0, nf);
    const Philox x = philox4x32_10(0u, ordinal, epoch, BATCH_STREAM_ITEM, k0, k1);
    const int fi = ok ? (int)batch_mulhi(x.x[3], (unsigned)nf) : 0;
    if (m == 0) {
        quarter[item] = (int)(x.x[0] >> 30);
        u[item] = 6.0 + 28.0 * ((double)x.x[1] * 0x1p-32);
        file[item] = fi;
    }
    if (m >= M) return;
    long long first = 0;
    unsigned n = 0;
    unsigned idx = 0;
    if (ok && batch_file(s, f0, nf, fi, first, n) && n > 0) {
        if ((unsigned)M > n) {
            const Philox w = philox4x32_10((unsigned)m >> 2, ordinal, epoch, BATCH_STREAM_OCC, k0, k1);
            const unsigned word = (m & 3) == 0 ? w.x[0] : (m & 3) == 1 ? w.x[1] : (m & 3) == 2 ? w.x[2] : w.x[3];
            idx = batch_mulhi(word, n);
        } else if (n > 1) {
            idx = batch_permute((unsigned)m, n, philox4x32_10(0u, ordinal, epoch, BATCH_STREAM_OCC, k0, k1));
        }
    }
    index[(size_t)item * M + m] = (int)idx;
}

struct BatchAsmArgs {
    GigaBatchSet s;
    const int* rows;
    const int* quarter;
    const double* u;
    const int* file;
    const int* index;
    float* x;
    float* pos;
    float* pos_occ;
    float* label;
    float* rot;
    float* width;
    float* occ;
    int B, M, augment;
    int occ_blocks;                           // occupancy workgroups per item (at least one: lane 0 writes the pose)
    float size_f, size_p;                     // size as float32, and rounded to the points' type
};

__device__ __forceinline__ void batch_grid_rows(const BatchAsmArgs& a, unsigned blk) {
    const int item = (int)(blk / BATCH_GRID_BLOCKS);
    const int o4 = (int)(blk % BATCH_GRID_BLOCKS) * BATCH_BLOCK + (int)threadIdx.x;
    if (o4 >= BATCH_VOX4) return;
    const int row = a.rows[item];
    int scene = 0, f0 = 0, nf = 0;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (batch_scene(a.s, row, scene, f0, nf)) {
        const float* __restrict__ src = a.s.grids + (size_t)scene * BATCH_VOX;
        if (!a.augment) {
            out = *reinterpret_cast<const float4*>(src + 4 * o4);
        } else {
            const int ij = o4 / BATCH_ROW4, k0 = (o4 % BATCH_ROW4) * 4;
            const int i = ij / BATCH_RES, j = ij % BATCH_RES;
            const int q = a.quarter[item] & 3;
            const int si = q == 0 ? i : q == 1 ? j : q == 2 ? BATCH_RES - i : BATCH_RES - j;
            const int sj = q == 0 ? j : q == 1 ? BATCH_RES - i : q == 2 ? BATCH_RES - j : i;
            if (si >= 0 && si < BATCH_RES && sj >= 0 && sj < BATCH_RES) {
                const double z_off = a.u[item] - (double)a.s.row_pos[(size_t)row * 3 + 2];
                const float* __restrict__ line = src + (si * BATCH_RES + sj) * BATCH_RES;
                float v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double c = (double)(k0 + t) - z_off;
                    const bool in = c >= 0.0 && c <= (double)(BATCH_RES - 1);           // (false for a NaN shift)
                    const int sk = in ? (int)floor(c + 0.5) : 0;                       // 0 .. 39 where `in`
                    v[t] = in ? line[sk] : 0.f;
                }
                out = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    *reinterpret_cast<float4*>(a.x + (size_t)item * BATCH_VOX + 4 * o4) = out;
}

__device__ void batch_pose(const BatchAsmArgs& a, int item, int row, bool ok) {
    float p[3] = {0.f, 0.f, 0.f}, r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, w = 0.f, lab = 0.f;
    if (ok) {
        const float* pm = a.s.row_pos + (size_t)row * 3;
        w = __fdiv_rn(a.s.row_width[row], a.size_f);
        lab = a.s.row_label[row];
        if (!a.augment) {
            for (int c = 0; c < 3; ++c) p[c] = __fsub_rn(__fdiv_rn(pm[c], a.size_f), 0.5f);
            for (int c = 0; c < 8; ++c) r[c] = a.s.row_rotations[(size_t)row * 8 + c];
        } else {
            const int q = a.quarter[item] & 3;
            const double z_off = a.u[item] - (double)pm[2];
            const double dx = (double)pm[0] - 20.0, dy = (double)pm[1] - 20.0;
            const double rx = q == 0 ? dx : q == 1 ? -dy : q == 2 ? -dx : dy;
            const double ry = q == 0 ? dy : q == 1 ? dx : q == 2 ? -dy : -dx;
            const double t[3] = {rx + 20.0, ry + 20.0, (double)pm[2] + z_off};
            for (int c = 0; c < 3; ++c) p[c] = (float)(t[c] / a.s.size - 0.5);
            const float* qm = a.s.row_quat + (size_t)row * 4;
            const double bx = qm[0], by = qm[1], bz = qm[2], bw = qm[3];
            const double norm = sqrt(((bx * bx + by * by) + bz * bz) + bw * bw);
            const double ox = bx / norm, oy = by / norm, oz = bz / norm, ow = bw / norm;
            const double s = q == 0 ? 0.0 : q == 1 ? 0.7071067811865475 : q == 2 ? 1.0 : 0.7071067811865476;
            const double c = q == 0 ? 1.0 : q == 1 ? 0.7071067811865476 : q == 2 ? 6.123233995736766e-17 : -0.7071067811865475;
            const double r0[4] = {c * ox - s * oy, c * oy + s * ox, c * oz + s * ow, c * ow - s * oz};
            r[0] = (float)r0[0]; r[1] = (float)r0[1]; r[2] = (float)r0[2]; r[3] = (float)r0[3];
            r[4] = (float)r0[1]; r[5] = (float)-r0[0]; r[6] = (float)r0[3]; r[7] = (float)-r0[2];
        }
    }
    for (int c = 0; c < 3; ++c) a.pos[(size_t)item * 3 + c] = p[c];
    for (int c = 0; c < 8; ++c) a.rot[(size_t)item * 8 + c] = r[c];
    a.width[item] = w;
    a.label[item] = lab;
}

__device__ __forceinline__ void batch_occupancy(const BatchAsmArgs& a, unsigned blk) {
    const int item = (int)(blk / (unsigned)a.occ_blocks);
    const int m = (int)(blk % (unsigned)a.occ_blocks) * BATCH_BLOCK + (int)threadIdx.x;
    if (m >= a.M && m != 0) return;
    const int row = a.rows[item];
    int scene = 0, f0 = 0, nf = 0;
    const bool ok = batch_scene(a.s, row, scene, f0, nf);
    if (m == 0) batch_pose(a, item, row, ok);
    if (m >= a.M) return;
    float p[3] = {0.f, 0.f, 0.f}, o = 0.f;
    long long first = 0;
    unsigned n = 0;
    const size_t at = (size_t)item * a.M + m;
    if (ok && batch_file(a.s, f0, nf, a.file[item], first, n)) {
        const int idx = a.index[at];
        if (idx >= 0 && (unsigned)idx < n) {
            const size_t g = (size_t)first + (size_t)idx;
            o = (float)a.s.occ[g];
            if (a.s.point_dtype == GIGA_BATCH_POINTS_F16) {
                const __half* src = static_cast<const __half*>(a.s.points) + 3 * g;
                for (int c = 0; c < 3; ++c) {
                    const __half quot = __float2half_rn(__fdiv_rn(__half2float(src[c]), a.size_p));
                    p[c] = __half2float(__float2half_rn(__fsub_rn(__half2float(quot), 0.5f)));
                }
            } else {
                const float* src = static_cast<const float*>(a.s.points) + 3 * g;
                for (int c = 0; c < 3; ++c) p[c] = __fsub_rn(__fdiv_rn(src[c], a.size_p), 0.5f);
            }
        }
    }
    for (int c = 0; c < 3; ++c) a.pos_occ[3 * at + c] = p[c];
    a.occ[at] = o;
}

__global__ __launch_bounds__(BATCH_BLOCK) void batch_assemble_kernel(BatchAsmArgs a) {
    const unsigned grid_blocks = (unsigned)a.B * BATCH_GRID_BLOCKS;
    if (blockIdx.x < grid_blocks) batch_grid_rows(a, blockIdx.x);
    else batch_occupancy(a, blockIdx.x - grid_blocks);
}

// `size` rounded once to float16 (round to nearest even, as numpy's conversion of a Python float), returned as a float
static float batch_size_as_half(double size) {
    const _Float16 h = (_Float16)size;
    return (float)h;
}

static int launch_batch_assemble(const GigaBatchSet& set, const int32_t* rows, const int32_t* quarter, const double* u, const int32_t* file,
                                 const int32_t* index, int B, int M, int augment, float* x, float* pos, float* pos_occ, float* label,
                                 float* rotations, float* width, float* occ, hipStream_t s) {
    BatchAsmArgs a{};
    a.s = set;
    a.rows = rows; a.quarter = quarter; a.u = u; a.file = file; a.index = index;
    a.x = x; a.pos = pos; a.pos_occ = pos_occ; a.label = label; a.rot = rotations; a.width = width; a.occ = occ;
    a.B = B; a.M = M; a.augment = augment != 0;
    a.occ_blocks = M > 0 ? (M + BATCH_BLOCK - 1) / BATCH_BLOCK : 1;
    a.size_f = (float)set.size;
    a.size_p = set.point_dtype == GIGA_BATCH_POINTS_F16 ? batch_size_as_half(set.size) : a.size_f;
    const unsigned long long blocks = (unsigned long long)B * (unsigned long long)(BATCH_GRID_BLOCKS + a.occ_blocks);
    if (blocks >= (1ull << 31)) return -1;
    GIGA_LAUNCH(batch_assemble_kernel, dim3((unsigned)blocks), dim3(BATCH_BLOCK), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

// everything about the set that can be checked on the host; `all`: giga_batch_assemble reads every array, giga_batch_draw the tables
// behind the file sizes only
static int batch_set_check(const GigaBatchSet* set, bool all) {
    if (!set) return -1;
    if (set->n_scenes < 0 || set->n_rows < 0 || set->n_files < 0 || set->n_points < 0) return -1;
    if (!set->row_scene || !set->scene_files || !set->file_points) return -1;
    if (all) {
        if (!set->grids || !set->row_pos || !set->row_quat || !set->row_rotations || !set->row_width || !set->row_label ||
            !set->points || !set->occ)
            return -1;
        if (set->point_dtype != GIGA_BATCH_POINTS_F32 && set->point_dtype != GIGA_BATCH_POINTS_F16) return -1;
        if (!finite_f64(set->size) || !(set->size > 0.0)) return -1;
        if (reinterpret_cast<uintptr_t>(set->grids) % 16 != 0) return -1;
    }
    if (set->scene_files_host) {
        const int32_t* f = set->scene_files_host;
        if (f[0] != 0 || f[set->n_scenes] != set->n_files) return -1;
        for (int i = 0; i < set->n_scenes; ++i)
            if (f[i + 1] < f[i]) return -1;
    }
    if (set->file_points_host) {
        const int64_t* p = set->file_points_host;
        if (p[0] != 0 || p[set->n_files] != set->n_points) return -1;
        for (int i = 0; i < set->n_files; ++i)
            if (p[i + 1] < p[i] || p[i + 1] - p[i] >= (1LL << 31)) return -1;
    }
    return 0;
}

static bool batch_shape_ok(int B, int M) {
    return B >= 0 && M >= 0 && B <= GIGA_BATCH_MAX_ITEMS && (long long)B * M < (1LL << 31);
}

int giga_batch_draw(const GigaBatchSet* set, const int32_t* ordinals, const int32_t* rows, int B, int M, int epoch,
                    unsigned long long seed, int32_t* quarter, double* u, int32_t* file, int32_t* index, void* stream) {
    if (!batch_shape_ok(B, M) || epoch < 0) return -1;
    if (const int rc = batch_set_check(set, false)) return rc;
    if (B == 0) return 0;
    if (!ordinals || !rows) return -1;
    if (!quarter || !u || !file || (M > 0 && !index)) return -6;
    const int per = M > 0 ? (M + BATCH_BLOCK - 1) / BATCH_BLOCK : 1;
    GIGA_LAUNCH(batch_draw_kernel, dim3((unsigned)per, (unsigned)B), dim3(BATCH_BLOCK), 0, static_cast<hipStream_t>(stream), *set,
                ordinals, rows, M, (unsigned)epoch, (unsigned)seed, (unsigned)(seed >> 32), quarter, u, file, index);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_batch_assemble(const GigaBatchSet* set, const int32_t* rows, const int32_t* quarter, const double* u, const int32_t* file,
                        const int32_t* index, int B, int M, int augment, float* x, float* pos, float* pos_occ, float* label,
                        float* rotations, float* width, float* occ, void* stream) {
    if (!batch_shape_ok(B, M)) return -1;
    if (const int rc = batch_set_check(set, true)) return rc;
    if (B == 0) return 0;
    if (!rows || !file || (M > 0 && !index) || (augment && (!quarter || !u))) return -1;
    if (!x || !pos || !label || !rotations || !width || (M > 0 && (!pos_occ || !occ))) return -6;
    if (reinterpret_cast<uintptr_t>(x) % 16 != 0) return -1;
    return launch_batch_assemble(*set, rows, quarter, u, file, index, B, M, augment, x, pos, pos_occ, label, rotations, width, occ,
                                 static_cast<hipStream_t>(stream));
}

}  // extern "C"
