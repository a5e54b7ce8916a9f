// MISE (multiresolution isosurface extraction) on the device: the counterpart of utils/libmise/mise.pyx as
// conv_onet/generation.py:125-142 drives it.  B scenes, independent octrees, one set of launches per round.
//
// State per scene, R = resolution0 << depth, N = R + 1 samples per axis (all of it in the caller's workspace):
//   state  one byte per lattice sample, linear index (i N + j) N + k: 0 absent, 1 unknown (created, not evaluated), 2 known.
//          Four samples share a 32-bit word; the stride of a scene is rounded up to whole words.
//   values one float per sample, defined where state == 2.
//   tree   one byte per voxel of the levels 0 .. depth-1 (level l: (resolution0 << l)^3 voxels of edge 1 << (depth - l), z fastest,
//          each level padded to whole words): bit 0 leaf, bit 1 "a known point of the closed cube has v >= thr", bit 2 "... v <= thr",
//          bit 3 inner node, bit 4 fresh (a leaf made by this update, its bits not collected yet).
//          Voxels of the last level are never subdivided and need no byte: a unit cell whose ancestors are all inner nodes is one.
//   dirty  one byte per run of 1024 samples (the 256 state words of one workgroup): "may hold an unknown point" (set where a point
//          is created, cleared by a count that finds none).  Most of the lattice is never touched; count and emit skip such runs.
//
// The two bits of a leaf are those of ALL known points of its closed cube (loc <= p <= loc + edge), which is what mise.pyx:197-218
// recomputes in every round by visiting the 8 unit cells p + {-1,0}^3 of every known point.  Here they are kept: a point's value
// never changes and a leaf with both bits is subdivided in the same update, so the bits of a leaf that stays are still right, and
// an update only adds what is new.  update = mark (the queried points become known and OR their bits into the <= 8 leaves around
// them) -> subdivide (every leaf with both bits becomes an inner node: 8 children, 27 lattice points created where absent) ->
// fresh (each new child collects the bits of the known points of its closed cube).  All bits are complete before the first
// subdivision of an update, and a child made by it is not looked at before the next, as in the reference.  Work per update is
// proportional to the new points and new leaves, not to all known points.
// query = count -> scan -> emit over the state words, in ascending linear index: no atomic append, two runs give the same bytes.
// to_dense = three sweeps (x, y, z) that copy the previous sample into a NaN one, NaN being "no value yet" as in mise.pyx:130-164.
// Integer work on one byte per sample: no MFMA, no LDS beyond the scan's few words.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_scan.h"
#include "giga_ws.h"
#include <cmath>
#include <cstdint>

namespace giga {

constexpr int MISE_BLOCK = 256;
constexpr int MISE_WAVES = MISE_BLOCK / 64;
constexpr unsigned MISE_UNKNOWN = 1, MISE_KNOWN = 2;
constexpr unsigned MISE_LEAF = 1, MISE_POS = 2, MISE_NEG = 4, MISE_INNER = 8, MISE_FRESH = 16;
constexpr int MISE_MAX_DEPTH = 9;                           // (1 << depth) < GIGA_MISE_MAX_N = 513

struct MiseDims {
    int res0, depth;
    unsigned N;              // samples per axis
    unsigned n3;             // N^3
    unsigned words;          // state words per scene
    unsigned nblk;           // workgroups per scene of the count / emit kernels
    unsigned tree;           // tree bytes per scene (whole words)
    unsigned off[MISE_MAX_DEPTH + 1];   // first tree byte of level l; off[depth] = tree
};

__host__ __device__ __forceinline__ unsigned mise_level_bytes(int res0, int l) {
    const unsigned n = (unsigned)res0 << l;
    return (n * n * n + 3u) & ~3u;
}

MiseDims mise_dims(int res0, int depth) {
    MiseDims d;
    d.res0 = res0; d.depth = depth;
    d.N = ((unsigned)res0 << depth) + 1;
    d.n3 = d.N * d.N * d.N;
    d.words = (d.n3 + 3) / 4;
    d.nblk = (d.words + MISE_BLOCK - 1) / MISE_BLOCK;
    d.tree = 0;
    for (int l = 0; l <= MISE_MAX_DEPTH; ++l) {
        d.off[l] = d.tree;
        if (l < depth) d.tree += mise_level_bytes(res0, l);
    }
    return d;
}

// counts | blk | dirty | state | tree | values : all but the values are cleared by one fill at init
struct MiseWs { size_t counts, blk, dirty, state, tree, values, total; };
static MiseWs mise_workspace(int B, int res0, int depth) {
    const MiseDims d = mise_dims(res0, depth);
    WsLayout L;
    MiseWs w;
    w.counts = L.take<int>((size_t)B);
    w.blk = L.take<unsigned>((size_t)B * d.nblk);
    w.dirty = L.take<unsigned char>((size_t)B * d.nblk);
    w.state = L.take<unsigned>((size_t)B * d.words);
    w.tree = L.take<unsigned char>((size_t)B * d.tree);
    w.values = L.take<float>((size_t)B * d.n3);
    w.total = L.total;
    return w;
}

__global__ __launch_bounds__(MISE_BLOCK) void mise_fill_kernel(unsigned* __restrict__ p, size_t n, unsigned v) {
    for (size_t i = (size_t)blockIdx.x * MISE_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * MISE_BLOCK) p[i] = v;
}

// the (res0+1)^3 coarse lattice points become unknown, the res0^3 voxels of level 0 leaves
__global__ __launch_bounds__(MISE_BLOCK) void mise_seed_kernel(unsigned char* __restrict__ state, unsigned char* __restrict__ tree,
                                                               unsigned char* __restrict__ dirty, MiseDims d) {
    const unsigned t = blockIdx.x * MISE_BLOCK + threadIdx.x, scene = blockIdx.y;
    const unsigned c = (unsigned)d.res0 + 1, S = 1u << d.depth;
    if (t < c * c * c) {
        const unsigned k = t % c, r = t / c, j = r % c, i = r / c;
        const unsigned idx = ((i * S) * d.N + j * S) * d.N + k * S;
        state[(size_t)scene * d.words * 4 + idx] = (unsigned char)MISE_UNKNOWN;
        dirty[(size_t)scene * d.nblk + idx / (4 * MISE_BLOCK)] = 1;
    }
    if (t < (unsigned)(d.res0 * d.res0 * d.res0)) tree[(size_t)scene * d.tree + t] = (unsigned char)MISE_LEAF;
}

// ---- query: count / scan / emit over the state words ------------------------------------------------------------------------
__device__ __forceinline__ unsigned unknown_mask(const unsigned* __restrict__ state, const MiseDims& d, unsigned scene, unsigned t) {
    return t < d.words ? state[(size_t)scene * d.words + t] & 0x01010101u : 0u;     // states are 0, 1, 2: bit 0 <=> unknown
}

__global__ __launch_bounds__(MISE_BLOCK) void mise_count_kernel(const unsigned* __restrict__ state, MiseDims d,
                                                                unsigned* __restrict__ blk, unsigned char* __restrict__ dirty) {
    __shared__ unsigned wsum[MISE_WAVES];
    const unsigned t = blockIdx.x * MISE_BLOCK + threadIdx.x, scene = blockIdx.y;
    const size_t run = (size_t)scene * d.nblk + blockIdx.x;
    if (!dirty[run]) {                                      // (the same byte for the whole workgroup)
        if (threadIdx.x == 0) blk[run] = 0;
        return;
    }
    unsigned total;
    block_excl<MISE_WAVES>((unsigned)__popc(unknown_mask(state, d, scene, t)), wsum, total);
    if (threadIdx.x == 0) {
        blk[run] = total;
        if (!total) dirty[run] = 0;
    }
}

__global__ __launch_bounds__(MISE_BLOCK) void mise_emit_kernel(const unsigned* __restrict__ state, MiseDims d,
                                                               const unsigned* __restrict__ blk, const int* __restrict__ ws_counts,
                                                               const unsigned char* __restrict__ dirty, int* __restrict__ query,
                                                               unsigned long long cap, int* __restrict__ shortfall) {
    __shared__ unsigned wsum[MISE_WAVES];
    const unsigned t = blockIdx.x * MISE_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (shortfall && blockIdx.x == 0 && threadIdx.x == 0) shortfall[scene] = scan_shortfall((unsigned)ws_counts[scene], cap);
    if (!dirty[(size_t)scene * d.nblk + blockIdx.x]) return;
    const unsigned m = unknown_mask(state, d, scene, t);
    unsigned total;
    unsigned long long at = block_excl<MISE_WAVES>((unsigned)__popc(m), wsum, total);
    if (!m) return;
    at += blk[(size_t)scene * d.nblk + blockIdx.x];
    int* q = query + (size_t)scene * cap;
#pragma unroll
    for (unsigned e = 0; e < 4; ++e)
        if (m >> (8 * e) & 1u) {
            if (at < cap) q[at] = (int)(4 * t + e);
            ++at;
        }
}

// points [B][cap][3] of the query list, through the per-axis table; entries past a scene's count repeat its first point (sample 0
// for a scene that has none), so that the decoder launch over [B][cap] reads only valid points
__global__ __launch_bounds__(MISE_BLOCK) void mise_points_kernel(const int* __restrict__ query, unsigned long long cap,
                                                                 const int* __restrict__ ws_counts, MiseDims d,
                                                                 const float* __restrict__ lin, float* __restrict__ points) {
    const unsigned long long i = (unsigned long long)blockIdx.x * MISE_BLOCK + threadIdx.x;
    const unsigned scene = blockIdx.y;
    if (i >= cap) return;
    const unsigned long long n = (unsigned)ws_counts[scene];
    const int* q = query + (size_t)scene * cap;
    unsigned idx = i < n ? (unsigned)q[i] : (n ? (unsigned)q[0] : 0u);
    if (idx >= d.n3) idx = 0;
    const unsigned k = idx % d.N, r = idx / d.N, j = r % d.N, x = r / d.N;
    float* o = points + ((size_t)scene * cap + i) * 3;
    o[0] = lin[x]; o[1] = lin[j]; o[2] = lin[k];
}

// ---- update ------------------------------------------------------------------------------------------------------------------
// the queried points become known, and each ORs its bits into the <= 8 leaves around it (the leaf of a unit cell is looked for from
// level depth-1 upwards: an absent voxel means a coarser leaf, an inner node at depth-1 that the cell is a leaf of the last level)
__global__ __launch_bounds__(MISE_BLOCK) void mise_mark_kernel(const float* __restrict__ vals, const int* __restrict__ query,
                                                               unsigned long long cap, const int* __restrict__ ws_counts, MiseDims d,
                                                               double thr, unsigned char* __restrict__ state, float* __restrict__ values,
                                                               unsigned* __restrict__ tree) {
    const unsigned long long n_at = (unsigned long long)blockIdx.x * MISE_BLOCK + threadIdx.x;
    const unsigned scene = blockIdx.y;
    const unsigned long long n = (unsigned)ws_counts[scene];
    if (n_at >= cap || n_at >= n) return;
    const unsigned idx = (unsigned)query[(size_t)scene * cap + n_at];
    if (idx >= d.n3) return;
    unsigned char* s = state + (size_t)scene * d.words * 4 + idx;
    if (*s != MISE_UNKNOWN) return;                       // (a list that is not this state's query changes nothing)
    const float val = vals[(size_t)scene * cap + n_at];
    values[(size_t)scene * d.n3 + idx] = val;
    *s = (unsigned char)MISE_KNOWN;
    const double v = (double)val;
    const unsigned bits = (v >= thr ? MISE_POS : 0u) | (v <= thr ? MISE_NEG : 0u);
    if (!bits) return;                                     // NaN
    unsigned* tw = tree + (size_t)scene * (d.tree / 4);
    const unsigned char* tb = reinterpret_cast<const unsigned char*>(tw);
    const int R = (int)d.N - 1;
    const int k = (int)(idx % d.N);
    const unsigned r = idx / d.N;
    const int j = (int)(r % d.N), i = (int)(r / d.N);
    unsigned last = 0xffffffffu;
    for (int c = 0; c < 8; ++c) {
        const int x = i - (c >> 2 & 1), y = j - (c >> 1 & 1), z = k - (c & 1);           // the unit cell p + {-1,0}^3
        if ((unsigned)x >= (unsigned)R || (unsigned)y >= (unsigned)R || (unsigned)z >= (unsigned)R) continue;
        for (int l = d.depth - 1; l >= 0; --l) {
            const int sh = d.depth - l;
            const unsigned nl = (unsigned)d.res0 << l;
            const unsigned at = d.off[l] + (((unsigned)(x >> sh) * nl + (unsigned)(y >> sh)) * nl + (unsigned)(z >> sh));
            const unsigned b = tb[at];
            if (b & MISE_INNER) break;
            if (b & MISE_LEAF) {
                if (at != last && (b & bits) != bits) atomicOr(tw + (at >> 2), bits << (8 * (at & 3u)));
                last = at;
                break;
            }
        }
    }
}

__device__ __forceinline__ int mise_word_level(const MiseDims& d, unsigned t) {
    int l = 0;
    while (l < d.depth - 1 && 4 * t >= d.off[l + 1]) ++l;
    return l;
}

// one thread per tree word: every leaf with both bits becomes an inner node, its stored children fresh leaves
__global__ __launch_bounds__(MISE_BLOCK) void mise_subdivide_kernel(unsigned* __restrict__ tree, MiseDims d,
                                                                    unsigned char* __restrict__ state, unsigned char* __restrict__ dirty) {
    const unsigned t = blockIdx.x * MISE_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (t >= d.tree / 4) return;
    unsigned char* tb = reinterpret_cast<unsigned char*>(tree + (size_t)scene * (d.tree / 4));
    const unsigned w = reinterpret_cast<const unsigned*>(tb)[t];
    if (!(w & (w >> 1) & (w >> 2) & 0x01010101u)) return;   // no byte with leaf, pos and neg
    const int l = mise_word_level(d, t);
    const unsigned off = d.off[l], nl = (unsigned)d.res0 << l, off2 = d.off[l + 1], nl2 = nl * 2;
    const unsigned s = 1u << (d.depth - l), half = s >> 1;
    unsigned char* st = state + (size_t)scene * d.words * 4;
    for (unsigned e = 0; e < 4; ++e) {
        if ((w >> (8 * e) & 0xffu) != (MISE_LEAF | MISE_POS | MISE_NEG)) continue;
        const unsigned at = 4 * t + e;
        tb[at] = (unsigned char)MISE_INNER;
        const unsigned v = at - off;
        const unsigned vz = v % nl, r = v / nl, vy = r % nl, vx = r / nl;
        if (l + 1 < d.depth)
            for (unsigned c = 0; c < 8; ++c)
                tb[off2 + ((2 * vx + (c >> 2 & 1)) * nl2 + 2 * vy + (c >> 1 & 1)) * nl2 + 2 * vz + (c & 1)] =
                    (unsigned char)(MISE_LEAF | MISE_FRESH);
        for (unsigned a = 0; a < 3; ++a)
            for (unsigned bb = 0; bb < 3; ++bb)
                for (unsigned c = 0; c < 3; ++c) {
                    const unsigned idx = ((vx * s + a * half) * d.N + vy * s + bb * half) * d.N + vz * s + c * half;
                    if (st[idx] == 0) {                                // (every writer of this launch writes the same bytes)
                        st[idx] = (unsigned char)MISE_UNKNOWN;
                        dirty[(size_t)scene * d.nblk + idx / (4 * MISE_BLOCK)] = 1;
                    }
                }
    }
}

// one thread per tree word: a fresh leaf collects the bits of the points of its closed cube that are known already (its corners,
// and what finer neighbours put on its faces); later points reach it through mise_mark_kernel
__global__ __launch_bounds__(MISE_BLOCK) void mise_fresh_kernel(unsigned* __restrict__ tree, MiseDims d,
                                                                const unsigned char* __restrict__ state, const float* __restrict__ values,
                                                                double thr) {
    const unsigned t = blockIdx.x * MISE_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (t >= d.tree / 4) return;
    unsigned char* tb = reinterpret_cast<unsigned char*>(tree + (size_t)scene * (d.tree / 4));
    const unsigned w = reinterpret_cast<const unsigned*>(tb)[t];
    if (!(w & 0x10101010u)) return;
    const int l = mise_word_level(d, t);
    const unsigned off = d.off[l], nl = (unsigned)d.res0 << l, s = 1u << (d.depth - l);
    const unsigned char* st = state + (size_t)scene * d.words * 4;
    const float* val = values + (size_t)scene * d.n3;
    for (unsigned e = 0; e < 4; ++e) {
        if (!(w >> (8 * e) & MISE_FRESH)) continue;
        const unsigned at = 4 * t + e, v = at - off;
        const unsigned vz = v % nl, r = v / nl, vy = r % nl, vx = r / nl;
        unsigned bits = 0;
        for (unsigned a = 0; a <= s && bits != (MISE_POS | MISE_NEG); ++a)
            for (unsigned bb = 0; bb <= s; ++bb)
                for (unsigned c = 0; c <= s; ++c) {
                    const unsigned idx = ((vx * s + a) * d.N + vy * s + bb) * d.N + vz * s + c;
                    if (st[idx] & MISE_KNOWN) {
                        const double x = (double)val[idx];
                        bits |= (x >= thr ? MISE_POS : 0u) | (x <= thr ? MISE_NEG : 0u);
                    }
                }
        tb[at] = (unsigned char)(MISE_LEAF | bits);         // (the only writer of this byte in this launch)
    }
}

// ---- to_dense ----------------------------------------------------------------------------------------------------------------
// sweep along x: out = value (0 for a point that is still unknown, mise.pyx:350-355) or NaN, a NaN sample takes out[i-1]
__global__ __launch_bounds__(MISE_BLOCK) void mise_dense_x_kernel(const unsigned char* __restrict__ state, const float* __restrict__ values,
                                                                  MiseDims d, float* __restrict__ out) {
    const unsigned t = blockIdx.x * MISE_BLOCK + threadIdx.x, scene = blockIdx.y;
    const unsigned plane = d.N * d.N;
    if (t >= plane) return;
    const unsigned char* s = state + (size_t)scene * d.words * 4;
    const float* v = values + (size_t)scene * d.n3;
    float* o = out + (size_t)scene * d.n3;
    float prev = NAN;
    for (unsigned i = 0; i < d.N; ++i) {
        const size_t at = (size_t)i * plane + t;
        const unsigned b = s[at];
        float x = (b & MISE_KNOWN) ? v[at] : (b == MISE_UNKNOWN ? 0.0f : NAN);
        if (x != x) x = prev;
        o[at] = x;
        prev = x;
    }
}

__global__ __launch_bounds__(MISE_BLOCK) void mise_dense_y_kernel(MiseDims d, float* __restrict__ out) {
    const unsigned t = blockIdx.x * MISE_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (t >= d.N * d.N) return;
    const unsigned k = t % d.N, i = t / d.N;
    float* o = out + (size_t)scene * d.n3 + (size_t)i * d.N * d.N + k;
    float prev = o[0];
    for (unsigned j = 1; j < d.N; ++j) {
        float x = o[(size_t)j * d.N];
        if (x != x) {
            x = prev;
            if (x == x) o[(size_t)j * d.N] = x;
        }
        prev = x;
    }
}

// one wave per row along z
__global__ __launch_bounds__(MISE_BLOCK) void mise_dense_z_kernel(MiseDims d, float* __restrict__ out) {
    const unsigned lane = threadIdx.x & 63, row = blockIdx.x * MISE_WAVES + (threadIdx.x >> 6), scene = blockIdx.y;
    if (row >= d.N * d.N) return;                           // whole waves leave together
    float* o = out + (size_t)scene * d.n3 + (size_t)row * d.N;
    float carry = NAN;
    for (unsigned base = 0; base < d.N; base += 64) {
        const unsigned k = base + lane;
        const bool in = k < d.N;
        float x = in ? o[k] : 0.0f;
        const bool hole = in && x != x;
        const unsigned long long have = __ballot(in && !hole) & ((2ull << lane) - 1ull);   // valid lanes at or below this one
        const int src = have ? 63 - __clzll((long long)have) : (int)lane;
        const float y = __shfl(x, src, 64);
        if (hole) {
            x = have ? y : carry;
            if (x == x) o[k] = x;
        }
        carry = __shfl(x, 63, 64);
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
static int launch_mise_init(int B, int res0, int depth, uint8_t* ws, hipStream_t s) {
    const MiseDims d = mise_dims(res0, depth);
    const MiseWs w = mise_workspace(B, res0, depth);
    const size_t nwords = w.values / 4;                     // counts, workgroup sums, dirty, state, tree
    const unsigned blocks = (unsigned)((nwords + MISE_BLOCK - 1) / MISE_BLOCK < 65536 ? (nwords + MISE_BLOCK - 1) / MISE_BLOCK : 65536);
    GIGA_LAUNCH(mise_fill_kernel, dim3(blocks), dim3(MISE_BLOCK), 0, s, reinterpret_cast<unsigned*>(ws), nwords, 0u);
    const unsigned c = (unsigned)res0 + 1;
    GIGA_LAUNCH(mise_seed_kernel, dim3((c * c * c + MISE_BLOCK - 1) / MISE_BLOCK, B), dim3(MISE_BLOCK), 0, s, ws + w.state, ws + w.tree, ws + w.dirty, d);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

static int launch_mise_count(int B, int res0, int depth, uint8_t* ws, int* counts, hipStream_t s) {
    const MiseDims d = mise_dims(res0, depth);
    const MiseWs w = mise_workspace(B, res0, depth);
    unsigned* blk = reinterpret_cast<unsigned*>(ws + w.blk);
    GIGA_LAUNCH(mise_count_kernel, dim3(d.nblk, B), dim3(MISE_BLOCK), 0, s, reinterpret_cast<const unsigned*>(ws + w.state), d, blk,
                ws + w.dirty);
    // the scene's total goes to the workspace copy too: emit, points and mark read it there
    GIGA_LAUNCH(scene_offsets_kernel<unsigned>, dim3(B), dim3(SCAN_BLOCK), 0, s, blk, d.nblk, reinterpret_cast<int*>(ws + w.counts), counts);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

static int launch_mise_emit(int B, int res0, int depth, const uint8_t* ws, int* query, size_t cap, int* shortfall, const float* lin,
                            float* points, hipStream_t s) {
    const MiseDims d = mise_dims(res0, depth);
    const MiseWs w = mise_workspace(B, res0, depth);
    const int* ws_counts = reinterpret_cast<const int*>(ws + w.counts);
    GIGA_LAUNCH(mise_emit_kernel, dim3(d.nblk, B), dim3(MISE_BLOCK), 0, s, reinterpret_cast<const unsigned*>(ws + w.state), d,
                reinterpret_cast<const unsigned*>(ws + w.blk), ws_counts, ws + w.dirty, query, (unsigned long long)cap, shortfall);
    if (points && cap > 0)
        GIGA_LAUNCH(mise_points_kernel, dim3((unsigned)((cap + MISE_BLOCK - 1) / MISE_BLOCK), B), dim3(MISE_BLOCK), 0, s, query,
                    (unsigned long long)cap, ws_counts, d, lin, points);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

static int launch_mise_update(const float* values, const int* query, size_t cap, int B, int res0, int depth, double thr, uint8_t* ws,
                              hipStream_t s) {
    const MiseDims d = mise_dims(res0, depth);
    const MiseWs w = mise_workspace(B, res0, depth);
    unsigned* tree = reinterpret_cast<unsigned*>(ws + w.tree);
    float* vals = reinterpret_cast<float*>(ws + w.values);
    const dim3 tgrid((d.tree / 4 + MISE_BLOCK - 1) / MISE_BLOCK, B);
    if (cap > 0)
        GIGA_LAUNCH(mise_mark_kernel, dim3((unsigned)((cap + MISE_BLOCK - 1) / MISE_BLOCK), B), dim3(MISE_BLOCK), 0, s, values, query,
                    (unsigned long long)cap, reinterpret_cast<const int*>(ws + w.counts), d, thr, ws + w.state, vals, tree);
    GIGA_LAUNCH(mise_subdivide_kernel, tgrid, dim3(MISE_BLOCK), 0, s, tree, d, ws + w.state, ws + w.dirty);
    GIGA_LAUNCH(mise_fresh_kernel, tgrid, dim3(MISE_BLOCK), 0, s, tree, d, ws + w.state, vals, thr);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

static int launch_mise_to_dense(int B, int res0, int depth, const uint8_t* ws, float* grid, hipStream_t s) {
    const MiseDims d = mise_dims(res0, depth);
    const MiseWs w = mise_workspace(B, res0, depth);
    const unsigned plane = d.N * d.N;
    GIGA_LAUNCH(mise_dense_x_kernel, dim3((plane + MISE_BLOCK - 1) / MISE_BLOCK, B), dim3(MISE_BLOCK), 0, s, ws + w.state,
                reinterpret_cast<const float*>(ws + w.values), d, grid);
    GIGA_LAUNCH(mise_dense_y_kernel, dim3((plane + MISE_BLOCK - 1) / MISE_BLOCK, B), dim3(MISE_BLOCK), 0, s, d, grid);
    GIGA_LAUNCH(mise_dense_z_kernel, dim3((plane + MISE_WAVES - 1) / MISE_WAVES, B), dim3(MISE_BLOCK), 0, s, d, grid);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

// 0 when the tree shape is supported, else the error code
static int mise_shape_check(int B, int res0, int depth) {
    if (B < 0 || res0 < 1 || depth < 1 || depth > 30) return -1;
    if (((long long)res0 << depth) + 1 > GIGA_MISE_MAX_N) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    const long long N = ((long long)res0 << depth) + 1;
    if ((long long)B * N * N * N >= (1LL << 31)) return -1;                           // sample numbers are 32-bit
    return 0;
}

size_t giga_mise_workspace_bytes(int B, int resolution0, int depth) {
    if (B <= 0 || mise_shape_check(B, resolution0, depth) != 0) return 0;
    return mise_workspace(B, resolution0, depth).total;
}

int giga_mise_init(int B, int resolution0, int depth, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_init(B, resolution0, depth, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

int giga_mise_count(int B, int resolution0, int depth, void* workspace, size_t workspace_bytes, int32_t* counts, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace || !counts) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_count(B, resolution0, depth, static_cast<uint8_t*>(workspace), counts, static_cast<hipStream_t>(stream));
}

int giga_mise_emit(int B, int resolution0, int depth, const void* workspace, size_t workspace_bytes, int32_t* query, size_t cap,
                   int32_t* shortfall, const float* lin, float* points, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace || (points && !lin)) return -1;
    if (cap > 0 && !query) return -6;
    if ((unsigned long long)B * cap >= (1ull << 31)) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_emit(B, resolution0, depth, static_cast<const uint8_t*>(workspace), query, cap, shortfall, lin, points,
                            static_cast<hipStream_t>(stream));
}

int giga_mise_update(const float* values, const int32_t* query, size_t cap, int B, int resolution0, int depth, double threshold,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (!(threshold == threshold)) return -1;
    if (B == 0) return 0;
    if (!workspace || (cap > 0 && (!values || !query))) return -1;
    if ((unsigned long long)B * cap >= (1ull << 31)) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_update(values, query, cap, B, resolution0, depth, threshold, static_cast<uint8_t*>(workspace),
                              static_cast<hipStream_t>(stream));
}

int giga_mise_to_dense(int B, int resolution0, int depth, const void* workspace, size_t workspace_bytes, float* grid, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace || !grid) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_to_dense(B, resolution0, depth, static_cast<const uint8_t*>(workspace), grid, static_cast<hipStream_t>(stream));
}

}  // extern "C"
