// csrc/lbm_group.inc.hpp — the gathers of an in-process group of strips (lbm_group_get_* / _drain_* / _pending, include/lbm_hip.h): what a
// caller of lbm_group_step reads back as ONE lattice. Every function calls the per-member entry points one after the other on the calling
// thread, as lbm_group_initialise does (no device code, no stream, no group thread of its own), and combines what they return with the
// routines of lbm_gather.hpp and nothing else. (part of the one host translation unit lbm_hip.hip, which includes it after its C-ABI)
#pragma once

namespace {

StripRows strip_rows(const lbm_ctx* c) { return {(size_t)c->nx, (size_t)c->p.ny, (size_t)c->p.y_start, (size_t)c->nyl}; }

// the value of a host-side quantity that every member must hold alike (`what`: its name in the message), or LBM_ERR_ARG
template <typename Get>
int common_value(lbm_ctx** cs, int n, const char* what, Get get) {
    const int v0 = get(cs[0]);
    for (int k = 1; k < n; ++k)
        if (get(cs[k]) != v0) return fail(LBM_ERR_ARG, "the strips of the group disagree on %s: strip 0 has %d, strip %d has %d", what, v0, k, get(cs[k]));
    return v0;
}

// All or nothing: a drain looks at every member's ring BEFORE the first member is drained. The members must hold the same number of
// samples and — where the host keeps them (frames, probes) — the same iterations for the `m` oldest; returns how many of the `m` are
// there, or LBM_ERR_ARG with every ring as it was. (Equal whenever lbm_group_step was the only thing that stepped the group.)
template <typename E>
int rings_agree(lbm_ctx** cs, int n, DeviceRing<E> lbm_ctx::*ring, int m, const char* samples) {
    char what[96];
    snprintf(what, sizeof(what), "the number of pending %s", samples);
    const int count = common_value(cs, n, what, [&](const lbm_ctx* c) { return (c->*ring).ix.count; });
    if (count < 0) return count;
    m = std::max(0, std::min(m, count));
    std::vector<int> t0((size_t)m), tk((size_t)m);
    (cs[0]->*ring).oldest_timesteps(m, t0.data());
    for (int k = 1; k < n; ++k) {
        (cs[k]->*ring).oldest_timesteps(m, tk.data());
        for (int j = 0; j < m; ++j)
            if (tk[(size_t)j] != t0[(size_t)j])
                return fail(LBM_ERR_ARG, "the strips of the group disagree on the iteration of the pending %s (number %d: strip 0 has %d, strip %d has %d); nothing was drained",
                            samples, j, t0[(size_t)j], k, tk[(size_t)j]);
    }
    return m;
}

// Strip k's rows of a force log into the group's: strip 0 gives the iterations (and bodies), every strip its partial sums. The two force
// logs carry their iterations in device memory only, so this comparison comes after the copy: a mismatch says that the rows are gone.
template <typename Row>
int add_force_rows(Row* total, const Row* part, int rows, int k, const char* log) {
    for (int r = 0; r < rows; ++r) {
        if (k == 0) total[r] = part[r];
        else if (part[r].timestep != total[r].timestep)
            return fail(LBM_ERR_ARG, "the strips of the group disagree on the iteration of row %d of the %s (strip 0 has %d, strip %d has %d): the drained rows are gone",
                        r, log, total[r].timestep, k, part[r].timestep);
        accumulate(&total[r].fx, &part[r].fx, 1, k == 0);
        accumulate(&total[r].fy, &part[r].fy, 1, k == 0);
    }
    return LBM_OK;
}

}  // namespace

extern "C" {

int lbm_group_first_unstable_step(lbm_ctx** cs, int n, int* t_out) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!t_out) return fail(LBM_ERR_ARG, "null argument");
    int first = -1;
    for (int k = 0; k < n; ++k) {
        int t = -1;
        if ((rc = lbm_first_unstable_step(cs[k], &t))) return rc;
        if (t >= 0 && (first < 0 || t < first)) first = t;
    }
    *t_out = first;
    return LBM_OK;
}

int lbm_group_max_velocity_sq(lbm_ctx** cs, int n, double* out) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!out) return fail(LBM_ERR_ARG, "null argument");
    double m = 0.0;
    for (int k = 0; k < n; ++k) {
        double v = 0.0;
        if ((rc = lbm_max_velocity_sq(cs[k], &v))) return rc;
        m = k == 0 ? v : std::max(m, v);
    }
    *out = m;
    return LBM_OK;
}

int lbm_group_get_forces(lbm_ctx** cs, int n, double* fx, double* fy) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    double f[2] = {0.0, 0.0}, part[2];
    for (int k = 0; k < n; ++k) {
        if ((rc = lbm_get_forces(cs[k], &part[0], &part[1]))) return rc;
        accumulate(f, part, 2, k == 0);
    }
    if (fx) *fx = f[0];
    if (fy) *fy = f[1];
    return LBM_OK;
}

int lbm_group_drain_force_log(lbm_ctx** cs, int n, lbm_force_row* rows, int max_rows) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!rows && max_rows > 0) return fail(LBM_ERR_ARG, "null argument");
    const int m = rings_agree(cs, n, &lbm_ctx::force_log, INT_MAX, "force-log rows");
    if (m < 0) return m;
    if (max_rows < m) return fail(LBM_ERR_ARG, "force log holds %d rows, buffer takes %d", m, max_rows);
    std::vector<lbm_force_row> part((size_t)std::max(m, 1));
    for (int k = 0; k < n; ++k) {
        if ((rc = lbm_drain_force_log(cs[k], part.data(), m)) < 0) return rc;
        if ((rc = add_force_rows(rows, part.data(), m, k, "force log"))) return rc;
    }
    return m;
}

int lbm_group_get_body_forces(lbm_ctx** cs, int n, double* fxy) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!fxy) return fail(LBM_ERR_ARG, "null argument");
    const int B = common_value(cs, n, "the number of bodies", [](const lbm_ctx* c) { return c->body_n; });
    if (B < 0) return B;
    std::vector<double> part(2 * (size_t)std::max(B, 1));
    for (int k = 0; k < n; ++k) {
        if ((rc = lbm_get_body_forces(cs[k], part.data()))) return rc;
        accumulate(fxy, part.data(), 2 * (size_t)B, k == 0);
    }
    return LBM_OK;
}

int lbm_group_drain_body_force_log(lbm_ctx** cs, int n, lbm_body_force_row* rows, int max_rows) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!rows && max_rows > 0) return fail(LBM_ERR_ARG, "null argument");
    const int B = common_value(cs, n, "the number of bodies", [](const lbm_ctx* c) { return c->body_n; });
    if (B < 1) return B;                                       // (an error, or no labels: nothing to drain)
    const int m = rings_agree(cs, n, &lbm_ctx::body_log, max_rows / B, "body-force samples");      // whole samples only
    if (m < 1) return m;
    std::vector<lbm_body_force_row> part((size_t)B * m);
    for (int k = 0; k < n; ++k) {
        if ((rc = lbm_drain_body_force_log(cs[k], part.data(), B * m)) < 0) return rc;
        if ((rc = add_force_rows(rows, part.data(), B * m, k, "body force log"))) return rc;
    }
    return B * m;
}

int lbm_group_get_macros(lbm_ctx** cs, int n, double* rho, double* ux, double* uy) {
    int rc = check_group(cs, n, true);
    for (int k = 0; k < n && !rc; ++k) {
        const size_t off = plane_offset(strip_rows(cs[k]));
        rc = lbm_get_macros(cs[k], rho ? rho + off : nullptr, ux ? ux + off : nullptr, uy ? uy + off : nullptr);
    }
    return rc;
}

int lbm_group_get_populations(lbm_ctx** cs, int n, int which, double* aos) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!aos) return fail(LBM_ERR_ARG, "null argument");
    std::vector<double> part;
    for (int k = 0; k < n; ++k) {
        const StripRows s = strip_rows(cs[k]);
        const size_t row = (s.nx + 2) * Q;
        part.resize(row * (s.rows + 2));
        if ((rc = lbm_get_populations(cs[k], which, part.data()))) return rc;
        stack_populations(aos, part.data(), row, s, k == 0, k == n - 1);
    }
    return LBM_OK;
}

int lbm_group_stats_samples(lbm_ctx** cs, int n) {
    const int rc = check_group(cs, n, true);
    return rc ? rc : common_value(cs, n, "the number of statistics samples", [](const lbm_ctx* c) { return c->stats_n; });
}

int lbm_group_get_stat_sums(lbm_ctx** cs, int n, double* sums6) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!sums6) return fail(LBM_ERR_ARG, "null argument");
    std::vector<double> part;
    for (int k = 0; k < n; ++k) {
        const StripRows s = strip_rows(cs[k]);
        part.resize(6 * s.rows * s.nx);
        if ((rc = lbm_get_stat_sums(cs[k], part.data()))) return rc;
        stack_planes(sums6, part.data(), 6, s);
    }
    return LBM_OK;
}

int lbm_group_stats_restore(lbm_ctx** cs, int n, const double* sums6, int samples) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (!sums6) return fail(LBM_ERR_ARG, "null argument");
    std::vector<double> part;
    for (int k = 0; k < n; ++k) {
        const StripRows s = strip_rows(cs[k]);
        part.resize(6 * s.rows * s.nx);
        unstack_planes(part.data(), sums6, 6, s);
        if ((rc = lbm_stats_restore(cs[k], part.data(), samples))) return rc;
    }
    return LBM_OK;
}

int lbm_group_frames_pending(lbm_ctx** cs, int n) {
    const int rc = check_group(cs, n, true);
    return rc ? rc : rings_agree(cs, n, &lbm_ctx::frames, INT_MAX, "frames");
}

int lbm_group_probes_pending(lbm_ctx** cs, int n) {
    const int rc = check_group(cs, n, true);
    return rc ? rc : rings_agree(cs, n, &lbm_ctx::probes, INT_MAX, "probe samples");
}

int lbm_group_drain_frames(lbm_ctx** cs, int n, int* timesteps, float* frames, int max_frames) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (max_frames < 0 || (max_frames > 0 && !frames)) return fail(LBM_ERR_ARG, "lbm_group_drain_frames: null argument or max_frames < 0");
    const int kf = common_value(cs, n, "the frame stride k", [](const lbm_ctx* c) { return c->frames_k; });
    if (kf < 0) return kf;
    const int m = rings_agree(cs, n, &lbm_ctx::frames, max_frames, "frames");
    if (m < 1) return m;                                       // (an error, or nothing pending: frames never begun, too)
    std::vector<float> part;
    for (int k = 0; k < n; ++k) {
        const StripRows s = coarsen(strip_rows(cs[k]), kf);
        const size_t per = 4 * s.rows * s.nx, whole = 4 * s.ny * s.nx;
        part.resize((size_t)m * per);
        if ((rc = lbm_drain_frames(cs[k], k == 0 ? timesteps : nullptr, part.data(), m)) < 0) return rc;
        for (int j = 0; j < m; ++j) stack_planes(frames + (size_t)j * whole, part.data() + (size_t)j * per, 4, s);
    }
    return m;
}

int lbm_group_drain_probes(lbm_ctx** cs, int n, int* timesteps, double* vals, int max_samples) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (max_samples < 0 || (max_samples > 0 && !vals)) return fail(LBM_ERR_ARG, "lbm_group_drain_probes: null argument or max_samples < 0");
    const int pn = common_value(cs, n, "the number of probes", [](const lbm_ctx* c) { return c->probe_n; });
    if (pn < 0) return pn;
    const int m = rings_agree(cs, n, &lbm_ctx::probes, max_samples, "probe samples");
    if (m < 1) return m;                                       // (an error, or nothing pending: probes never begun, too)
    std::vector<double> part(3 * (size_t)pn * m);
    for (int k = 0; k < n; ++k) {
        if ((rc = lbm_drain_probes(cs[k], k == 0 ? timesteps : nullptr, part.data(), m)) < 0) return rc;
        accumulate(vals, part.data(), part.size(), k == 0);
    }
    return m;
}

/* TEST HOOK (no device needed): the routines of lbm_gather.hpp on caller-supplied per-strip arrays: see include/lbm_hip.h. */
int lbm_debug_gather(int what, int n, const int* bounds2, int nx, int ny, int k, int planes, void* const* parts, void* whole) {
    if (what < 0 || what > 4 || n < 1 || !bounds2 || !parts || !whole || nx < 1 || ny < 1 || k < 1 || planes < 1) return fail(LBM_ERR_ARG, "bad argument");
    for (int i = 0; i < n; ++i) {
        const int y0 = bounds2[2 * i], rows = bounds2[2 * i + 1];
        if (!parts[i] || y0 < 0 || rows < 1 || y0 + rows > ny) return fail(LBM_ERR_ARG, "strip %d: null array or rows [%d, %d) outside [0, %d)", i, y0, y0 + rows, ny);
        const StripRows fine{(size_t)nx, (size_t)ny, (size_t)y0, (size_t)rows}, s = coarsen(fine, k);
        if (what == 0) stack_planes(static_cast<double*>(whole), static_cast<const double*>(parts[i]), planes, s);
        else if (what == 1) unstack_planes(static_cast<double*>(parts[i]), static_cast<const double*>(whole), planes, s);
        else if (what == 2) stack_planes(static_cast<float*>(whole), static_cast<const float*>(parts[i]), planes, s);
        else if (what == 3) stack_populations(static_cast<double*>(whole), static_cast<const double*>(parts[i]), (fine.nx + 2) * Q, fine, i == 0, i == n - 1);
        else accumulate(static_cast<double*>(whole), static_cast<const double*>(parts[i]), (size_t)nx * planes, i == 0);
    }
    return LBM_OK;
}

}  // extern "C"
