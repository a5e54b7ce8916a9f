// Host-only check of csrc/giga_dec_bwd_plan.h, for a sanitizer build (no HIP, no device):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dec_bwd_plan_check.cpp -o /tmp/dec_bwd_plan_check && /tmp/dec_bwd_plan_check
// For the case table of tests/dect_exact.py and a sweep of small B, N, M over every head set, both precisions, attached and detached:
// every region of every call lies inside the step's scratch, no two regions overlap (within a call or across the two calls), the
// launch list has as many entries as the calls' launches add up to, and every grid is within one workgroup per CU.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../giga_amd/csrc/giga_dec_bwd_plan.h"

using namespace giga;

struct Region { long long lo, hi; };

static long long g_checked = 0;

static bool check(int B, int N, int M, int hp, bool detach, bool bf16) {
    const TrainDecPlan t = train_dec_plan(B, N, M, hp, detach, bf16);
    std::vector<Region> r;
    int launches = 0;
    const DecBwdCall* calls[2] = {&t.occ, &t.grasp};
    const long long bases[2] = {t.occ_base, t.grasp_base};
    for (int k = 0; k < 2; ++k) {
        const DecBwdCall& c = *calls[k];
        if (!c.runs) { if (c.scratch_floats != 0) return false; continue; }
        launches += c.launches;
        if (c.grid_x < 1 || c.grid_x > 256 || c.grid_y < 1 || c.grid_x * c.grid_y > 256 * NHEADS || c.lds > 160 * 1024) return false;
        if (!bf16 && (c.nb_total * c.ksplit < 1 || (long long)c.ksplit * c.pts_per_block < c.P || c.pts_per_block % 32)) return false;
        if (c.gather && c.dcbuf_off < 0) return false;
        const size_t first = r.size();
        for (int h = 0; h < c.nheads; ++h) r.push_back({c.head_off + h * c.head_stride, c.head_off + (h + 1) * c.head_stride});
        if (c.cbuf_off >= 0) r.push_back({c.cbuf_off, c.cbuf_off + c.P * 96});
        if (c.pbuf_off >= 0) r.push_back({c.pbuf_off, c.pbuf_off + c.P * 32});
        if (c.dcbuf_off >= 0) r.push_back({c.dcbuf_off, c.dcbuf_off + c.P * 96});
        for (size_t i = first; i < r.size(); ++i) {
            if (r[i].lo < 0 || r[i].hi > c.scratch_floats) return false;
            r[i].lo += bases[k]; r[i].hi += bases[k];
        }
    }
    if (t.reduce) ++launches;
    if (launches != t.launches || launches > TRAIN_DEC_MAX_LAUNCHES) return false;
    for (int i = 0; i < t.launches; ++i)
        if (t.order[i] <= DBK_NONE || t.order[i] > DBK_DECT_REDUCE) return false;
    std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
    for (size_t i = 0; i < r.size(); ++i) {
        if (r[i].lo < 0 || r[i].hi > t.scratch_floats || r[i].hi < r[i].lo) return false;
        if (i && r[i - 1].hi > r[i].lo) return false;
    }
    ++g_checked;
    return true;
}

int main() {
    const int table[][4] = {{15, 1, 1, 1}, {15, 1, 33, 255}, {15, 3, 43, 256}, {15, 7, 3, 600}, {15, 2, 1, 4097}, {15, 16, 1, 2048},
                            {15, 17, 37, 2047}, {15, 32, 1, 2048}, {15, 33, 1, 2047}, {7, 5, 2, 0}, {8, 3, 0, 300}, {15, 4, 1, 256},
                            {7, 32, 340, 0}, {7, 32, 341, 0}, {8, 2, 0, 4096}, {8, 2, 0, 4097}};
    const int sizes[] = {0, 1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 4096, 4097};
    int bad = 0;
    for (int bf16 = 0; bf16 < 2; ++bf16)
        for (int detach = 0; detach < 2; ++detach) {
            for (const auto& c : table)
                if (!check(c[1], c[2], c[3], c[0], detach, bf16)) { std::printf("FAIL hp %d B %d N %d M %d detach %d bf16 %d\n", c[0], c[1], c[2], c[3], detach, bf16); ++bad; }
            for (int hp = 0; hp < 16; ++hp)
                for (int B : {1, 2, 3, 8, 33, 3072})
                    for (int N : sizes)
                        for (int M : sizes)
                            if (!check(B, N, M, hp, detach, bf16)) { std::printf("FAIL hp %d B %d N %d M %d detach %d bf16 %d\n", hp, B, N, M, detach, bf16); ++bad; }
        }
    std::printf("%lld plans checked, %d failed\n", g_checked, bad);
    return bad ? 1 : 0;
}
