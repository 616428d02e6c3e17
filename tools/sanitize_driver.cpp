// tools/sanitize_driver.cpp — the host-side logic that runs WITHOUT a GPU (the group threads' rendezvous with its error and time-out paths,
// the dry run of the strip choreography and its checker, the stacking arithmetic of the group gathers, the parser of the checkpoint head) under ThreadSanitizer and AddressSanitizer + UBSan: tools/sanitize_host.sh.
// (GPU AddressSanitizer is not available on this pool; the device code is covered by the parity tests.)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/lbm_hip.h"      // (lbm_ckpt_head and its two hooks)
extern "C" {
int lbm_debug_group_pool(int n, int rounds, int fail_strip, int fail_round, int stall_strip, int stall_round, int stall_ms, long timeout_ms, int repeat, int* rendezvous_out);
int lbm_debug_choreography(int nx, int ny, const int* bounds2, int nstrips, int precision, int transport, const char* options, const int* calls2, int ncalls, int dump, char* out, int cap);
int lbm_debug_p2p_matching(int nx, int ny, const int* bounds2, int nranks, int precision, const char* options, const char* options_rank1, const int* calls2, int ncalls, char* out, int cap);
int lbm_debug_gather(int what, int n, const int* bounds2, int nx, int ny, int k, int planes, void* const* parts, void* whole);
const char* lbm_last_error(void);
}
// The gather hook on exactly-sized heap arrays (an index past a strip's part or past the whole is a heap-buffer-overflow): strips of
// 12 + 16 + 20 rows of 8 cells; six double planes stacked and cut out again, four float planes at k = 4, the populations of 1 - 3
// strips, a sum. Returns the cases whose result is wrong.
static int gather_cases() {
    const int nx = 8, ny = 48, b[6] = {0, 12, 12, 16, 28, 20};
    int bad = 0;
    auto run = [&](int what, int n, int lattice_ny, int k, int planes, size_t per_row, int extra_rows, auto zero) {
        using E = decltype(zero);
        std::vector<std::vector<E>> parts;
        std::vector<void*> ptrs;
        const size_t part_planes = what == 3 || what == 4 ? 1 : (size_t)planes, whole_rows = what == 4 ? 1 : (size_t)(lattice_ny / k + extra_rows);
        for (int i = 0; i < n; ++i) {
            const size_t rows = what == 4 ? 1 : (size_t)(b[2 * i + 1] / k + extra_rows);
            parts.emplace_back(part_planes * rows * per_row);
            for (size_t q = 0; q < parts.back().size(); ++q) parts.back()[q] = (E)(1000 * (i + 1) + (int)(q % 997));
        }
        for (auto& p : parts) ptrs.push_back(p.data());
        std::vector<E> whole(part_planes * whole_rows * per_row, (E)-1);
        int rc = lbm_debug_gather(what, n, b, nx, lattice_ny, k, planes, ptrs.data(), whole.data());
        if (what == 0 && rc == 0) {      // and back: every part must come out as it went in
            std::vector<std::vector<E>> back = parts;
            for (size_t i = 0; i < back.size(); ++i) { std::fill(back[i].begin(), back[i].end(), (E)-2); ptrs[i] = back[i].data(); }
            rc = lbm_debug_gather(1, n, b, nx, lattice_ny, k, planes, ptrs.data(), whole.data());
            if (back != parts) ++bad;
        }
        for (E v : whole) if (v == (E)-1) { ++bad; break; }      // every element of the whole was written
        if (rc) ++bad;
    };
    run(0, 3, ny, 1, 6, nx, 0, 0.0);
    run(2, 3, ny, 4, 4, nx / 4, 0, 0.0f);
    for (int n = 1; n <= 3; ++n) run(3, n, b[2 * (n - 1)] + b[2 * n - 1], 1, 1, (size_t)(nx + 2) * 9, 2, 0.0);
    run(4, 3, ny, 1, 5, (size_t)nx * 5, 0, 0.0);
    return bad;
}
// The head of a checkpoint (csrc/lbm_ckpt.hpp) through lbm_debug_ckpt_save / lbm_debug_ckpt_load, every input an exactly-sized heap copy (a
// read past a truncated head is a heap-buffer-overflow): the 64 described runs — mask x profile x walls x schedule x {BGK, LES, TRT,
// forced}. Each head must load into its own description and take all its bytes; cut at every shorter length it must be refused with
// nothing taken; with any byte of its flag word set to any other value (fields announced that the bytes do not hold, unknown bits, two
// collision models) it must be refused. Then the digests from exactly-sized data. Returns the cases whose result is wrong.
static int ckpt_cases(int* cases_out) {
    int bad = 0, cases = 0;
    const int bases[4] = {0, 2, 4, 8};
    for (int k = 0; k < 64; ++k) {
        lbm_ckpt_head h{};
        h.nx = 128; h.ny = 32; h.local_ny = 32; h.steps_done = 11; h.tau = 0.6; h.inlet_velocity = 0.05;
        h.cylinder_x = 0.2; h.cylinder_y = 0.5; h.cylinder_radius = 0.125;
        h.has_mask = k & 1; h.has_profile = (k >> 1) & 1; h.has_walls = (k >> 2) & 1; h.has_sched = (k >> 3) & 1; h.collision = bases[k >> 4];
        h.mask_digest = 0x0123456789abcdefull; h.profile_digest = 0xfedcba9876543210ull; h.sched_digest = 0x0f1e2d3c4b5a6978ull;
        h.collision_param[0] = 0.17; h.collision_param[1] = -2.5e-6;
        h.walls[0] = 2.0; h.walls[1] = 0.05; h.walls[2] = 1.0;
        unsigned char full[LBM_CKPT_HEAD_MAX];
        const int n = lbm_debug_ckpt_save(&h, nullptr, nullptr, nullptr, 0, 0, full, (int)sizeof(full));
        if (n < 72) { ++bad; continue; }
        for (int len = 1; len <= n; ++len, ++cases) {
            const std::vector<unsigned char> cut(full, full + len);
            int used = -1;
            const int rc = lbm_debug_ckpt_load(cut.data(), len, &h, "x.ckpt", &used);
            if (len == n ? (rc != 0 || used != n) : (rc != -1 || used != 0 || !strstr(lbm_last_error(), "is not a checkpoint"))) ++bad;
        }
        for (int b = 72; full[7] == '3' && b < 80; ++b)
            for (int v = 0; v < 256; ++v) {
                if (full[b] == v) continue;
                std::vector<unsigned char> p(full, full + n);
                p[b] = (unsigned char)v;
                ++cases;
                if (lbm_debug_ckpt_load(p.data(), n, &h, "x.ckpt", nullptr) != -1) ++bad;
            }
    }
    lbm_ckpt_head h{};
    h.nx = 7; h.ny = 5; h.local_ny = 5;
    const std::vector<unsigned char> mask(35, 1);
    const std::vector<double> profile(5, 0.03), sched(3, 0.5);
    std::vector<unsigned char> out(LBM_CKPT_HEAD_MAX);
    const int n = lbm_debug_ckpt_save(&h, mask.data(), profile.data(), sched.data(), 3, 1, out.data(), (int)out.size());
    bad += n != 72 + 8 + 3 * 8 || !h.has_mask || !h.has_profile || !h.has_sched;
    bad += lbm_debug_ckpt_save(&h, nullptr, nullptr, nullptr, 0, 0, out.data(), (int)out.size() - 1) != -1;      // a buffer too small is refused
    *cases_out = cases + 2;
    return bad;
}
int main() {
    int passed = 0;
    int rc = lbm_debug_group_pool(8, 2000, -1, -1, -1, -1, 0, 0, 3, &passed);
    printf("clean: rc %d passed %d\n", rc, passed);
    rc = lbm_debug_group_pool(6, 40, 3, 17, -1, -1, 0, 0, 2, &passed);
    printf("fail: rc %d passed %d: %s\n", rc, passed, lbm_last_error());
    rc = lbm_debug_group_pool(4, 20, -1, -1, 2, 9, 700, 150, 1, &passed);
    printf("stall: rc %d passed %d: %s\n", rc, passed, lbm_last_error());
    int b[6] = {0, 100, 100, 100, 200, 100}, calls[2] = {40, 0};
    static char out[1 << 16];
    int bad = 0, runs = 0;
    const char* plans[] = {"fuse=3 pair_ty=12", "deep=1", "deep=3", "deep=7 arith=1", "deep=9"};
    for (const char* plan : plans)
        for (int dh = 0; dh < 3; ++dh)
            for (int ov = 0; ov < 3; ++ov)
                for (int transport = 0; transport < 2; ++transport) {
                    char opts[160];
                    snprintf(opts, sizeof(opts), "tune=0 nt=1 xcd=1 overlap=%d deep_halo=%d %s", ov, dh, plan);
                    rc = lbm_debug_choreography(256, 300, b, 3, 0, transport, opts, calls, 1, 0, out, sizeof(out));
                    bad += rc != 0; ++runs;
                }
    printf("choreography: %d dry runs, %d flagged or failed\n", runs, bad);
    int b8[16], bad2 = 0, runs2 = 0;
    for (int k = 0; k < 8; ++k) { b8[2 * k] = 128 * k; b8[2 * k + 1] = 128; }
    for (const char* plan : plans)
        for (int trim = 0; trim < 2; ++trim) {
            char opts[160];
            snprintf(opts, sizeof(opts), "tune=0 nt=1 xcd=1 overlap=1 deep_halo=1 halo_trim=%d trailing_pair=1 %s", trim, plan);
            rc = lbm_debug_p2p_matching(4096, 1024, b8, 8, 0, opts, nullptr, calls, 1, out, sizeof(out));
            bad2 += rc != 0; ++runs2;
        }
    printf("p2p matching: %d eight-rank dry runs, %d mismatching or failed\n", runs2, bad2);
    printf("group gathers: 6 cases through lbm_debug_gather, %d wrong\n", gather_cases());
    int ncases = 0;
    const int wrong = ckpt_cases(&ncases);
    printf("checkpoint heads: %d cases through lbm_debug_ckpt_save / lbm_debug_ckpt_load, %d wrong\n", ncases, wrong);
    return wrong != 0;      // (the script fails on a nonzero exit code)
}
