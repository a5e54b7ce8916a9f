// Host-only check of csrc/giga_enc_plan.h, for a sanitizer build (no HIP, no device):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/enc_plan_check.cpp -o /tmp/enc_plan_check && /tmp/enc_plan_check
// For every B in 1..3072, precision 0..3, every combination of the seven call flags, GIGA_WINOGRAD unset / 0 / 3 / 0x1FFF,
// GIGA_C32_FUSE unset / 0 / 1, 64 / 256 / 304 compute units and both values of slot_free: the workspace regions lie inside `total`,
// are 256-byte aligned and pairwise disjoint (XZ == YZ is the one documented alias), every grid is positive and the persistent grid
// is at most one workgroup per CU, `launches` is what `layers` / `nlayers` imply, and wino_mask has no bit of a 1x1 layer or beyond.
// Also: mega_groups at the image counts on both sides of each of its steps, and the two knobs as the environment gives them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../giga_amd/csrc/giga_enc_plan.h"

using namespace giga;

static long long g_checked = 0;

static bool check_workspace(int B, int precision) {
    const EncWs w = enc_workspace(B, precision);
    const size_t es = precision == 1 ? 2 : 4, n = 3 * (size_t)B;
    struct Region { size_t lo, hi; };
    std::vector<Region> r;
    auto add = [&](size_t off, size_t bytes) { r.push_back({off, off + bytes}); };
    add(w.P0, n * conv_in_elems(0) * es);
    const size_t outs[12] = {w.A0, w.S0, w.A1, w.S1, w.A2, w.S2, w.U0, w.A3, w.A4, w.U1, w.A5, w.A6};
    for (int l = 0; l < 12; ++l) add(outs[l], n * conv_out_elems(l) * es);
    add(w.Q0, n * conv_pool_elems(1) * es);
    add(w.Q1, n * conv_pool_elems(3) * es);
    add(w.YZ, (size_t)(4 + enc_nxp(B)) * B * RES * RES * CD * 4);
    add(w.SYNC, (size_t)MEGA_SYNC_WORDS * 4);
    add(w.MASK, (size_t)B * 8 * RES * 64 * 16);
    if (w.XZ != w.YZ) return false;
    for (const Region& x : r)
        if (x.lo % 256 || x.hi > w.total || x.hi <= x.lo) return false;
    std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i - 1].hi > r[i].lo) return false;
    return true;
}

static bool check_plan(const EncCall& c, int B, int cus, bool slot_free, const EncKnobs& k) {
    const EncPlan p = enc_plan(c, B, cus, -1, slot_free, k);
    ++g_checked;
    if (p.nimg != 3 * B || p.nlayers != (c.fold_final ? 12 : 13)) return false;
    if (p.ci_grid_x < 1 || p.ci_grid_y < 1 || p.ci_grid_z < 1 || p.ci_block != 64 * p.ci_nw || p.fin_grid < 1 || p.fin_block < 1) return false;
    if ((long long)p.ci_grid_x * p.ci_grid_y * p.ci_grid_z != 8LL * p.nxp * B || p.ci_sxw * p.ci_nw * p.nxp != RES) return false;
    if ((long long)p.fin_grid * p.fin_block * 4 < (long long)B * RES * RES * CD) return false;
    if (p.persistent) {
        if (cus != 256 || !slot_free || p.grid < 1 || p.grid > 256 || p.grid != 8 * p.groups || p.block < 64 || p.block > 1024) return false;
    } else if (p.grid || p.block || p.fused) return false;
    int launched = 0;
    for (int l = 0; l < NCONV; ++l) {
        const int f = p.layer_kernel[l];
        if ((f != ENC_LAYER_NONE) != (l < p.nlayers)) return false;
        launched += f != ENC_LAYER_NONE;
        if ((f == ENC_LAYER_CONV32) != (p.conv32 && l < p.nlayers)) return false;
        if ((f == ENC_LAYER_WINO || f == ENC_LAYER_UP) != ((p.wino_mask >> l & 1u) && l < p.nlayers)) return false;
    }
    if (p.launches != 2 + (p.persistent ? 1 : launched)) return false;
    for (int l = 0; l < 32; ++l)
        if ((p.wino_mask >> l & 1u) && (l >= NCONV || kConv[l].kind == CONV1 || c.precision != 0)) return false;
    if (((p.path & GIGA_PATH_WINOGRAD) != 0) != (p.wino_mask != 0) || ((p.path & GIGA_PATH_PERSISTENT) != 0) != (p.persistent != 0) ||
        ((p.path & GIGA_PATH_CONV32) != 0) != (p.conv32 != 0) || ((p.path & GIGA_PATH_FUSED_PAIRS) != 0) != (p.fused != 0)) return false;
    return true;
}

int main() {
    int bad = 0;
    const int images[7] = {8, 9, 16, 17, 24, 25, 9216}, groups[7] = {8, 16, 16, 24, 24, 32, 32};
    for (int i = 0; i < 7; ++i)
        if (mega_groups(images[i]) != groups[i]) { std::printf("FAIL mega_groups(%d)\n", images[i]); ++bad; }
    unsetenv("GIGA_WINOGRAD"); unsetenv("GIGA_C32_FUSE");
    if (enc_knobs_from_env().winograd != WINO_DEFAULT_MASK || enc_knobs_from_env().c32_fuse >= 0) { std::printf("FAIL knobs unset\n"); ++bad; }
    setenv("GIGA_WINOGRAD", "0x1FFF", 1); setenv("GIGA_C32_FUSE", "0", 1);
    if (enc_knobs_from_env().winograd != 0x1FFF || enc_knobs_from_env().c32_fuse != 0) { std::printf("FAIL knobs set\n"); ++bad; }
    for (int B = 1; B <= 3072; ++B)
        for (int prec = 0; prec < 4; ++prec)
            if (!check_workspace(B, prec)) { std::printf("FAIL workspace B %d precision %d\n", B, prec); ++bad; }
    const int flags[7] = {GIGA_FOLD_FINAL, GIGA_PERSIST_UNET, GIGA_LAYERWISE_UNET, GIGA_CONV32_UNET, GIGA_CONV16_UNET, GIGA_CONVIN_MASK, GIGA_DIRECT_CONV};
    const char* wino[4] = {nullptr, "0", "3", "0x1FFF"};
    const char* fuse[3] = {nullptr, "0", "1"};
    for (const char* wv : wino)
        for (const char* fv : fuse) {
            if (wv) setenv("GIGA_WINOGRAD", wv, 1); else unsetenv("GIGA_WINOGRAD");
            if (fv) setenv("GIGA_C32_FUSE", fv, 1); else unsetenv("GIGA_C32_FUSE");
            const EncKnobs k = enc_knobs_from_env();
            for (int prec = 0; prec < 4; ++prec)
                for (int fm = 0; fm < 128; ++fm) {
                    int word = prec;
                    for (int b = 0; b < 7; ++b) if (fm >> b & 1) word |= flags[b];
                    const EncCall c = enc_call_from_flags(word);
                    if (c.precision != prec) { std::printf("FAIL word %d\n", word); ++bad; continue; }
                    for (int cus : {64, 256, 304})
                        for (int slot = 0; slot < 2; ++slot)
                            for (int B = 1; B <= 3072; ++B)
                                if (!check_plan(c, B, cus, slot != 0, k)) {
                                    if (bad++ < 20) std::printf("FAIL B %d word %d cus %d slot_free %d GIGA_WINOGRAD %s GIGA_C32_FUSE %s\n", B, word, cus, slot, wv ? wv : "-", fv ? fv : "-");
                                }
                }
        }
    std::printf("%lld plans checked, %d failed\n", g_checked, bad);
    return bad ? 1 : 0;
}
