// csrc/lbm_ckpt.hpp — the head of a checkpoint file (lbm_save_state / lbm_load_state; SURVEY §8f-4: the reference keeps its state in
// memory only): what it says about a run (lbm_ckpt_head, include/lbm_hip.h), ONE table of its optional fields, and the three functions
// the table drives: serialise, parse, refuse. Plus the FNV-1a digests a head carries. Pure host C++ (no HIP call, no device): the
// library exports it through lbm_debug_ckpt_save / lbm_debug_ckpt_load (tests/test_ckpt_cpu.py, tools/sanitize_driver.cpp).
//
// THE FILE, little-endian, no padding:
//   offset  0  the magic, 8 characters: "LBMCKPT1", "LBMCKPT2" or "LBMCKPT3"
//           8  six 32-bit ints   nx, ny, y_start, local_ny, precision, steps_done
//          32  five doubles      tau, inlet_velocity, cylinder_x, cylinder_y, cylinder_radius
//          72  "LBMCKPT3" only:  a 64-bit word of flags, one bit per optional field that follows
//              the optional fields, in ascending order of their bits, 8-byte words each:
//                bit 0 (1)   1 word    the obstacle mask's digest             lbm_set_solid_mask / lbm_set_body_labels
//                bit 1 (2)   1 word    the inlet profile's digest             lbm_set_inlet_profile
//                bit 2 (4)   1 double  the Smagorinsky constant Cs            lbm_set_smagorinsky
//                bit 3 (8)   1 double  the TRT magic parameter                lbm_set_trt
//                bit 4 (16)  4 doubles south kind, south velocity, north kind, north velocity; where a wall is not no-slip: lbm_set_wall
//                bit 5 (32)  1 word    the inlet schedule's digest            lbm_set_inlet_schedule
//                bit 6 (64)  2 doubles the force {fx, fy}                     lbm_set_forcing
//                bit 7 (128) unassigned: a head that announces it is not a checkpoint
//                bit 8 (256) 4 doubles west kind, west value, east kind, east value; where a port is off its default: lbm_set_port
//                bit 9 (512) nothing   periodic y (the flag is the field)       lbm_set_periodic_y
//                bit 10 (1024) 2 doubles the MRT pair {bulk rate, magic}          lbm_set_mrt
//                bit 11 (2048) 2 doubles the outlet sponge {width, tau_end}       lbm_set_sponge
//              (the bits and sizes of the collision parameters are those of collision_models, lbm_plan.hpp; a context has one model)
//        then  the post-collision populations P_{steps_done} of the strip's interior, [9][local_ny][nx] in the element type
// "LBMCKPT2" is the fixed header, the mask's digest (no flags) and the populations; "LBMCKPT1" the fixed header and the populations.
// A context writes "LBMCKPT3" if it has any field but the mask, else "LBMCKPT2" with a mask, else "LBMCKPT1"; a reader also takes an
// "LBMCKPT3" file whose flags announce the mask alone, or nothing. The state is complete: ghost and solid cells are reconstructed by
// lbm_initialise; the iteration counter positions an inlet schedule after a restart. Statistics, frames and probes are not carried.
// The digests are 64-bit FNV-1a over 32-bit words (Fnv1a below): mask {nx, ny, one 0 / 1 word per cell, row 0 first}; profile {ny, the
// low and the high half of each velocity's bit pattern}; schedule {mode, n, the halves of each factor}.
// A context loads only a file that announces exactly the fields it has, with equal values (doubles compared as numbers) and an equal
// fixed header but for steps_done. The refusal names the first difference in this order: the collision models from the last row of
// collision_models to the first (sponge, MRT, forcing, TRT, Smagorinsky), the walls, periodic y, the ports, the inlet profile, the inlet schedule, the mask, the header.
#pragma once
#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <string>

#include "lbm_plan.hpp"
#include "../../include/lbm_hip.h"

namespace lbmk {

// ---- the digests ----
struct Fnv1a {
    unsigned long long d = 1469598103934665603ull;
    void mix(unsigned v) { d ^= v; d *= 1099511628211ull; }
    void mix_bits(double v) {      // the low half of the bit pattern, then the high one
        unsigned long long b;
        memcpy(&b, &v, sizeof(b));
        mix((unsigned)b); mix((unsigned)(b >> 32));
    }
};
inline unsigned long long mask_digest(const unsigned char* mask, int nx, int ny) {
    Fnv1a f;
    f.mix((unsigned)nx); f.mix((unsigned)ny);
    for (size_t k = 0; k < (size_t)nx * ny; ++k) f.mix(mask[k] ? 1u : 0u);
    return f.d;
}
inline unsigned long long profile_digest(const double* u, int ny) {
    Fnv1a f;
    f.mix((unsigned)ny);
    for (int y = 0; y < ny; ++y) f.mix_bits(u[y]);
    return f.d;
}
inline unsigned long long schedule_digest(const double* s, int n, int mode) {
    Fnv1a f;
    f.mix((unsigned)mode); f.mix((unsigned)n);
    for (int k = 0; k < n; ++k) f.mix_bits(s[k]);
    return f.d;
}

// ---- the refusals: what follows "checkpoint <path> was written " ----
inline std::string ckpt_text(const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    return b;
}
inline const char* wall_kind_name(int kind) { return kind == LBM_WALL_NOSLIP ? "no-slip" : kind == LBM_WALL_FREESLIP ? "free-slip" : "moving"; }

enum class CkptRefusal { file_lacks, context_lacks, differs };
struct CkptField;
using CkptPhrase = std::string (*)(const CkptField&, CkptRefusal, const lbm_ckpt_head& file, const lbm_ckpt_head& here);

// One optional field. It is present in a head where head.*key == present; its value is `words` 8-byte words at byte `value` of the head,
// doubles compared as numbers (`real`) or a digest compared bit for bit; `rank`: its place in the order of the refusals.
struct CkptField {
    unsigned long long bit = 0;
    int words = 0;
    int lbm_ckpt_head::*key = nullptr;
    int present = 0;
    size_t value = 0;
    bool real = false;
    int rank = 0;
    CkptPhrase phrase = nullptr;
    const char* noun = "";

    bool in(const lbm_ckpt_head& h) const { return h.*key == present; }
    bool differs(const lbm_ckpt_head& a, const lbm_ckpt_head& b) const {
        const char *pa = reinterpret_cast<const char*>(&a) + value, *pb = reinterpret_cast<const char*>(&b) + value;
        if (!real) return memcmp(pa, pb, 8 * (size_t)words) != 0;
        for (int w = 0; w < words; ++w) {
            double x, y;
            memcpy(&x, pa + 8 * w, 8); memcpy(&y, pb + 8 * w, 8);
            if (x != y) return true;
        }
        return false;
    }
};

inline std::string digest_refusal(const CkptField& f, CkptRefusal r, const lbm_ckpt_head&, const lbm_ckpt_head&) {
    return r == CkptRefusal::file_lacks      ? ckpt_text("without an %s; this context has one", f.noun)
           : r == CkptRefusal::context_lacks ? ckpt_text("with an %s; this context has none", f.noun)
                                             : ckpt_text("for a different %s", f.noun);
}
// (the words are the model's: collision_models)
inline std::string param_refusal(const CkptField& f, CkptRefusal r, const lbm_ckpt_head& file, const lbm_ckpt_head& here) {
    const CollisionModel& m = collision_model(f.present);
    const double *theirs = file.collision_param, *mine = here.collision_param;
    if (r == CkptRefusal::file_lacks) return ckpt_text("without a %s%s; this context has %s%s", m.param, m.none, m.value, param_text(m, mine[0], mine[1]).c_str());
    if (r == CkptRefusal::context_lacks) return ckpt_text("with %s %s%s; this context has none%s", m.param, m.value, param_text(m, theirs[0], theirs[1]).c_str(), m.none);
    return ckpt_text("with %s %s%s; this context has %s%s", m.param, m.value, param_text(m, theirs[0], theirs[1], "%.17g").c_str(), m.value,
                     param_text(m, mine[0], mine[1], "%.17g").c_str());
}
inline std::string walls_refusal(const CkptField&, CkptRefusal r, const lbm_ckpt_head& file, const lbm_ckpt_head& here) {
    const double *w = file.walls, *m = here.walls;
    if (r == CkptRefusal::file_lacks)
        return ckpt_text("with two no-slip walls; this context has a %s south wall and a %s north wall", wall_kind_name((int)m[0]), wall_kind_name((int)m[2]));
    if (r == CkptRefusal::context_lacks) return ckpt_text("with wall kinds %g (south) and %g (north); this context has two no-slip walls", w[0], w[2]);
    return ckpt_text("for different walls: south kind %g u = %.17g, north kind %g u = %.17g; this context has south kind %d u = %.17g, north kind %d u = %.17g",
                     w[0], w[1], w[2], w[3], (int)m[0], m[1], (int)m[2], m[3]);
}
// (a port's value with the fewest digits that read back exactly: 0.99, not 0.98999999999999999)
inline std::string shortest_text(double v) {
    char b[64];
    for (int digits = 1; digits <= 17; ++digits) {
        snprintf(b, sizeof(b), "%.*g", digits, v);
        if (strtod(b, nullptr) == v) break;
    }
    return b;
}
inline std::string ports_text(const double* p) {
    return ckpt_text("ports west kind %g value %s, east kind %g value %s", p[0], shortest_text(p[1]).c_str(), p[2], shortest_text(p[3]).c_str());
}
inline std::string ports_refusal(const CkptField&, CkptRefusal r, const lbm_ckpt_head& file, const lbm_ckpt_head& here) {
    if (r == CkptRefusal::file_lacks) return "with the default ports; this context has " + ports_text(here.ports);
    if (r == CkptRefusal::context_lacks) return "with " + ports_text(file.ports) + "; this context has the default ports";
    return "with " + ports_text(file.ports) + "; this context has " + ports_text(here.ports);
}

inline std::string periodic_refusal(const CkptField&, CkptRefusal r, const lbm_ckpt_head&, const lbm_ckpt_head&) {
    return r == CkptRefusal::file_lacks ? "without periodic y (two walls); this context has periodic y" : "with periodic y; this context has two walls";
}

// ---- the table: the six fields of the setters, and one per collision model that has a parameter ----
constexpr int CKPT_MODELS = (int)std::size(collision_models);
constexpr int ckpt_model_fields() {
    int n = 0;
    for (const CollisionModel& m : collision_models) n += m.ckpt_bit != 0;
    return n;
}
constexpr auto make_ckpt_fields(bool by_rank) {
    std::array<CkptField, 6 + ckpt_model_fields()> t{{
        {1, 1, &lbm_ckpt_head::has_mask, 1, offsetof(lbm_ckpt_head, mask_digest), false, CKPT_MODELS + 4, digest_refusal, "obstacle mask"},
        {2, 1, &lbm_ckpt_head::has_profile, 1, offsetof(lbm_ckpt_head, profile_digest), false, CKPT_MODELS + 2, digest_refusal, "inlet profile"},
        {16, 4, &lbm_ckpt_head::has_walls, 1, offsetof(lbm_ckpt_head, walls), true, CKPT_MODELS - 1, walls_refusal, "walls"},
        {32, 1, &lbm_ckpt_head::has_sched, 1, offsetof(lbm_ckpt_head, sched_digest), false, CKPT_MODELS + 3, digest_refusal, "inlet schedule"},
        {256, 4, &lbm_ckpt_head::has_ports, 1, offsetof(lbm_ckpt_head, ports), true, CKPT_MODELS + 1, ports_refusal, "ports"},
        {512, 0, &lbm_ckpt_head::has_periodic_y, 1, 0, false, CKPT_MODELS, periodic_refusal, "periodic y"},
    }};
    int k = 6;
    for (int i = 0; i < CKPT_MODELS; ++i) {
        const CollisionModel& m = collision_models[i];
        if (m.ckpt_bit) t[k++] = {m.ckpt_bit, m.nparam, &lbm_ckpt_head::collision, m.base, offsetof(lbm_ckpt_head, collision_param), true, CKPT_MODELS - 1 - i, param_refusal, m.param};
    }
    std::sort(t.begin(), t.end(), [by_rank](const CkptField& a, const CkptField& b) { return by_rank ? a.rank < b.rank : a.bit < b.bit; });
    return t;
}
constexpr auto ckpt_fields = make_ckpt_fields(false);          // in the order of the file
constexpr auto ckpt_refusal_order = make_ckpt_fields(true);    // in the order of the refusals

constexpr int CKPT_FIXED = 64;      // the bytes of the fixed header behind the magic: the head's leading members as they stand
static_assert(offsetof(lbm_ckpt_head, has_mask) == CKPT_FIXED && offsetof(lbm_ckpt_head, tau) == 24, "the fixed header is written as it lies in lbm_ckpt_head");
constexpr int ckpt_head_max() {
    int n = 8 + CKPT_FIXED + 8, model = 0;
    unsigned long long seen = 0;
    for (const CkptField& f : ckpt_fields) {
        if (!f.bit || (seen & f.bit)) return -1;       // (every field has a bit of its own)
        seen |= f.bit;
        if (f.key == &lbm_ckpt_head::collision) model = f.words > model ? f.words : model;      // (a head has one collision model: the longest)
        else n += 8 * f.words;
    }
    return n + 8 * model;
}
static_assert(ckpt_head_max() > 0 && ckpt_head_max() <= LBM_CKPT_HEAD_MAX, "LBM_CKPT_HEAD_MAX (include/lbm_hip.h) holds every head");

// ---- serialise, parse, refuse ----
// the head into out[LBM_CKPT_HEAD_MAX]; its length
inline int ckpt_serialise(const lbm_ckpt_head& h, unsigned char* out) {
    unsigned long long flags = 0;
    for (const CkptField& f : ckpt_fields)
        if (f.in(h)) flags |= f.bit;
    const int version = (flags & ~1ull) ? 3 : flags ? 2 : 1;
    memcpy(out, "LBMCKPT", 7);
    out[7] = (unsigned char)('0' + version);
    memcpy(out + 8, &h, CKPT_FIXED);
    int at = 8 + CKPT_FIXED;
    if (version == 3) { memcpy(out + at, &flags, 8); at += 8; }
    for (const CkptField& f : ckpt_fields)
        if (flags & f.bit) { memcpy(out + at, reinterpret_cast<const char*>(&h) + f.value, 8 * (size_t)f.words); at += 8 * f.words; }
    return at;
}

// the head in the first n bytes of a file; the bytes it takes, or 0: not a checkpoint (a short head, an unknown magic, a flag without a
// row in the table, two collision models)
inline int ckpt_parse(const unsigned char* p, int n, lbm_ckpt_head* out) {
    lbm_ckpt_head h{};
    int at = 8 + CKPT_FIXED;
    if (n < at || memcmp(p, "LBMCKPT", 7) != 0 || p[7] < '1' || p[7] > '3') return 0;
    memcpy(&h, p + 8, CKPT_FIXED);
    unsigned long long flags = p[7] == '2' ? 1 : 0;
    if (p[7] == '3') {
        if (n < at + 8) return 0;
        memcpy(&flags, p + at, 8);
        at += 8;
    }
    for (const CkptField& f : ckpt_fields) {
        if (!(flags & f.bit)) continue;
        if (h.*f.key != 0 || n < at + 8 * f.words) return 0;
        h.*f.key = f.present;
        memcpy(reinterpret_cast<char*>(&h) + f.value, p + at, 8 * (size_t)f.words);
        at += 8 * f.words;
        flags &= ~f.bit;
    }
    if (flags) return 0;
    *out = h;
    return at;
}

// a file's head against the loading context's: "" where they agree, else what follows "checkpoint <path> was written "
inline std::string ckpt_refusal(const lbm_ckpt_head& file, const lbm_ckpt_head& here) {
    for (const CkptField& f : ckpt_refusal_order) {
        const bool in_file = f.in(file), in_ctx = f.in(here);
        if (in_file != in_ctx) return f.phrase(f, in_ctx ? CkptRefusal::file_lacks : CkptRefusal::context_lacks, file, here);
        if (in_file && f.differs(file, here)) return f.phrase(f, CkptRefusal::differs, file, here);
    }
    if (file.nx != here.nx || file.ny != here.ny || file.y_start != here.y_start || file.local_ny != here.local_ny || file.precision != here.precision ||
        file.tau != here.tau || file.inlet_velocity != here.inlet_velocity || file.cylinder_x != here.cylinder_x || file.cylinder_y != here.cylinder_y ||
        file.cylinder_radius != here.cylinder_radius)
        return "for different parameters";
    return "";
}

}  // namespace lbmk
