// csrc/lbm_launch.inc.hpp — kernel arguments, layouts and the launchers of every step-kernel family (single iteration, fused tiles, deep LDS tiles, registers), forces
// (part of the one host translation unit lbm_hip.hip, which includes it in this place; round 4 split a 2 100-line file by concern)

// Periodic y (lbm_set_periodic_y) through the kernels' arguments: a periodic context's launches and samplers see the strip
// PERIODIC_PAD rows up (y_start + row_offset) in a lattice of rows_glob = ny + 2 PERIODIC_PAD rows — a strip in the middle of a taller
// lattice, which is the path every plan runs on an interior strip: no row is the domain's edge, so no wall rule, no one-sided
// difference and no clamp fires, and every row a launch or a sampler reaches (twelve halo rows; the frame's second ghost row lies within
// them) is a row of the lattice. The tables indexed by the global row (u_row, d_urow0, d_feqrow: rows_glob entries) and the geometry
// window (lbm_ctx::pmask) are filled from y mod ny to match (prepare_periodic, lbm_hip.hip). Walled: offset 0, ny rows, as ever.
constexpr int PERIODIC_PAD = 16;
static_assert(PERIODIC_PAD > GR + 1, "the offset covers the deepest reach of a launch and the lean test of a tile at the strip's first row");
inline int row_offset(const lbm_ctx* c) { return c->periodic_y ? PERIODIC_PAD : 0; }
inline int rows_glob(const lbm_ctx* c) { return c->p.ny + 2 * row_offset(c); }
inline int row_start(const lbm_ctx* c) { return c->p.y_start + row_offset(c); }
// the geometry the kernels read through MaskView: the user's mask, or — periodic y — the wrapped window of mask or disc
inline bool geom_masked(const lbm_ctx* c) { return c->has_mask || c->periodic_y; }
inline const HostMask& geom_mask(const lbm_ctx* c) { return c->periodic_y ? c->pmask : c->hmask; }

// The two walls as every argument block carries them (KArgs, MacroArgs): the packed kinds and the operands of wall_ks. The two ports
// (lbm_set_port) ride with them: their kinds in the spare bits of the same word (port_pack), their values cast once (port_ks).
template <typename T, typename A>
void fill_walls(const lbm_ctx* c, A& a) {
    a.walls = wall_pack(c->wall_kind[0], c->wall_kind[1]) | port_pack(c->port_kind[0], c->port_kind[1]);
    a.wk = wall_ks<T>(c->wall_kind[0], c->wall_u[0], c->wall_kind[1], c->wall_u[1]);
    a.pk = port_ks<T>(c->port_value[0], c->port_kind[1], c->port_value[1]);
}

// The launch-uniform values of the context's collision model in the slots of KArgs: the model's values formed from tau and its
// parameters (*_values) and stored through the slot map (put), both lbm_collision.hpp. Every slot the model does not own is zero; no
// kernel of the model reads it. The outlet sponge owns none: its rates are the table wp_x.
template <typename T>
void fill_collision(const lbm_ctx* c, KArgs<T>& a) {
    const double tau = c->p.tau, p1 = c->collision_param, p2 = c->collision_param2;
    clear_collision_slots(a);
    switch (c->collision) {
        case AR_STRICT: put(a, bgk_values<T>(tau)); break;
        case AR_STRICT_LES: put(a, les_values<T>(tau, p1)); break;
        case AR_STRICT_TRT: put(a, trt_values<T>(tau, p1)); break;
        case AR_STRICT_FORCED: put(a, forced_values<T>(tau, p1, p2)); break;
        case AR_STRICT_MRT: put(a, mrt_values<T>(tau, p1, p2)); break;
        default: break;
    }
}

// The inlet schedule's factor of iteration t in the element type, (T)s(t); 1 without a schedule (or before iteration 0).
template <typename T>
T inlet_scale(const lbm_ctx* c, int t) {
    if (!c->has_sched() || t < 0) return T(1);
    return (T)c->sched[(size_t)inlet_sched_index(t, (int)c->sched.size(), c->sched_mode)];
}

template <typename T>
KArgs<T> make_kargs(const lbm_ctx* c, int src, int dst, int t) {
    KArgs<T> a;
    a.src = static_cast<const T*>(c->buf[src]);
    a.dst = static_cast<T*>(c->buf[dst]);
    a.plane = (long)c->plane;
    a.pitch = c->pitch;
    a.xoff = c->xoff;
    a.nx = c->nx;
    a.ny_loc = c->nyl;
    a.ny_glob = rows_glob(c);
    a.y_start = row_start(c);
    a.cyl_x = c->cyl_x;
    a.cyl_y = c->cyl_y;
    a.cyl_r2 = (double)(c->cyl_r * c->cyl_r);
    if (geom_masked(c)) a.mv = c->mview;
    a.u_row = static_cast<const T*>(c->d_urow);
    a.unstable_t = c->d_unstable;
    a.t = t - c->tbase_host;
    a.t_base = c->d_tbase;
    a.y_lo = 0;
    a.y_cnt = c->nyl;
    a.y_lo2 = 0;
    a.y_cnt2 = 0;
    a.reverse = 0;
    fill_collision<T>(c, a);
    fill_walls<T>(c, a);
    a.sched = static_cast<const int*>(c->d_sched);
    a.wp_x = static_cast<const T*>(c->d_wpx);       // (lbm_initialise: upload_sponge; nullptr without a sponge)
    return a;
}

// Strides of the two layouts. Planar: plane stride = whole rows rounded up to k*64 KiB + 4 KiB (nine planes whose
// stride is a multiple of 64 KiB put the nine accesses of a wave on the same HBM channel group: 5.2-5.4 TB/s at +0
// vs 5.9-6.1 TB/s at +1..8 KiB, 4096x1024 fp64). Row-interleaved: the nine sub-rows of a lattice row are adjacent.
inline void configure_layout(lbm_ctx* c, int layout) {
    c->layout = layout;
    if (layout == 1) {
        c->plane = (size_t)c->pitch0;
        c->pitch = Q * c->pitch0;
        c->total = (size_t)c->pitch * (c->nyl + 2 * GR);
    } else {
        const size_t raw = (size_t)c->pitch0 * (c->nyl + 2 * GR) * c->esize;
        const size_t w = 65536;
        c->plane = ((raw + w - 1) / w * w + 4096) / c->esize;
        c->pitch = c->pitch0;
        c->total = (size_t)Q * c->plane;
    }
}
inline size_t buffer_bytes(const lbm_ctx* c) { return c->total * c->esize + 256; }  // +slack: displaced vector load

// The one place a collision model (lbm_ctx::collision, the base of a row of collision_models) becomes a template argument:
// f(std::integral_constant<int, base>) for the row whose base it is.
template <typename F>
void with_collision_base(int collision, F&& f) {
    [&]<size_t... I>(std::index_sequence<I...>) {
        (void)((collision == collision_models[I].base && (f(std::integral_constant<int, collision_models[I].base>{}), true)) || ...);
    }(std::make_index_sequence<std::size(collision_models)>{});
}

// Launch one step-family kernel over the local rows [a.y_lo, a.y_lo + a.y_cnt), with the context's collision model. Instantiated
// (lbm_step_k.hip) per model: MODE_STEP in both store policies and both arithmetic modes, MODE_COLLIDE_ONLY in both arithmetic modes;
// MODE_STREAM_ONLY once, under BGK (no collision in it).
template <typename T, int MODE>
void launch_rows(const lbm_ctx* c, const KArgs<T>& a, hipStream_t s) {
    const bool nt = (MODE == MODE_STEP) && c->use_nt;
    const bool fast = (MODE != MODE_STREAM_ONLY) && c->arith == AR_CONTRACTED;
    with_collision_base(MODE == MODE_STREAM_ONLY ? (int)AR_STRICT : c->collision, [&](auto arb) { launch_site<T, arb()>(a, MODE, nt, fast, s); });
}

// "deep" plans (deep_shapes, lbm_plan.hpp): rows of one band of tiles of a launch of `depth` iterations (the edge bands of a strip are
// one band each)
inline int deep_rows(const lbm_ctx* c, int id, int depth) {
    const RegionKind* k = deep_kind(id);
    return k ? col_tile_h(depth, col_rw(*k, (int)c->esize, c->arith != 0)) : deep_shape(id)->tile_h;
}
// K2Extra::small: the lean paths may address the buffer with 32-bit byte offsets (+ one row of slack). Also asked by lbm_debug_wave_plain.
inline bool buffer_small(const lbm_ctx* c) { return (c->total + (size_t)c->pitch) * c->esize + 1024 < (size_t(1) << 32); }
// A fused kernel over the local rows [a.y_lo, a.y_lo + a.y_cnt): iterations a.t .. a.t + depth - 1 (depth 2..8). LBM_ERR_ARG, and
// nothing queued: a deep launch of a depth the shape's row does not list (plan_launch reads the same row: it asks for none).
template <typename T>
int launch_fused_rows(const lbm_ctx* c, const KArgs<T>& a, int depth, hipStream_t s) {
    const int shape = c->deep;
    K2Extra<T> e;
    e.feq_in = static_cast<const T*>(c->d_feq);
    e.small = buffer_small(c) ? 1 : 0;
    e.xcd = c->xcd;
    e.nt = c->use_nt;
    e.ntl = c->use_ntl;
    const bool fast = c->arith == AR_CONTRACTED;
    bool ok = false;
    with_collision_base(c->collision, [&](auto arb) {
        if (!c->deep_now) { launch_tile<T, arb()>(a, e, depth, c->pair_ty, fast, s); ok = true; }
        // D iterations on a deep LDS tile (k_stepd_tile; whole-domain launches of small grids)
        else if (!deep_is_col(shape)) ok = depth == deep_depth(shape) && launch_deep<T, arb()>(a, e, shape, fast, s);
        // ... or with the lattice in registers (k_stepc_col, lbm_col.hip), on the shape's kind of region: an instantiation that is
        // not built is one refuse_deep has refused
        else with_row<std::size(region_kinds)>([&](size_t i) { return &region_kinds[i] == deep_kind(shape); }, [&](auto kind) {
            if constexpr (col_built<T, kind(), arb() | 1>()) { if (fast) ok = launch_col<T, kind(), arb() | 1>(a, e, depth, c->use_nt != 0, s); }
            if constexpr (col_built<T, kind(), arb()>()) { if (!fast) ok = launch_col<T, kind(), arb()>(a, e, depth, c->use_nt != 0, s); }
        });
    });
    return ok ? LBM_OK : fail(LBM_ERR_ARG, "deep %d has no launch of %d iterations here", shape, depth);
}
inline bool pair_possible(const lbm_ctx*) { return true; }   // partial tiles cover any nx
template <typename T>
int launch_step(lbm_ctx* c, int src, int dst, int t, int mode, hipStream_t s) {
    KArgs<T> a = make_kargs<T>(c, src, dst, t);
    a.reverse = ((mode == MODE_STEP || mode >= 100) && c->alternate && (c->launches_total & 1)) ? 1 : 0;
    switch (mode) {
        case MODE_STEP: launch_rows<T, MODE_STEP>(c, a, s); break;
        case 102: case 103: case 104: if (int rc = launch_fused_rows<T>(c, a, mode - 100, s)) return rc; break;     // iterations t .. t+1 / t+2 / t+3 (four: k_step4_tile, no strip faces)
        case MODE_COLLIDE_ONLY: launch_rows<T, MODE_COLLIDE_ONLY>(c, a, s); break;
        default: break;
    }
    HIPCHK(hipGetLastError());
    return LBM_OK;
}

// The snapshot's source as k_macros and k_stats take it: the lattice, the geometry and the inlet profile of this strip, read from
// `src`. One fill for both launches (do_macros, launch_stats), so that the two snapshots cannot differ in their arguments either.
// initial = 0 and no outputs: the caller sets what it needs. t: the iteration whose boundary rules the snapshot applies (`src` = P_t),
// which selects the inlet schedule's factor.
template <typename T>
MacroArgs<T> make_macro_args(const lbm_ctx* c, const void* src, int t) {
    MacroArgs<T> m;
    m.old = static_cast<const T*>(src);
    m.plane = (long)c->plane; m.pitch = c->pitch; m.xoff = c->xoff;
    m.nx = c->nx; m.ny_loc = c->nyl; m.ny_glob = rows_glob(c); m.y_start = row_start(c);
    m.cyl_x = c->cyl_x; m.cyl_y = c->cyl_y; m.cyl_r2 = (double)(c->cyl_r * c->cyl_r);
    if (geom_masked(c)) m.mv = c->mview;
    m.u_row = static_cast<const T*>(c->d_urow);
    fill_walls<T>(c, m);
    m.in_scale = inlet_scale<T>(c, t);
    m.forced = c->collision == AR_STRICT_FORCED ? 1 : 0;      // h = F/2 of the forced model's values; zeros, unread, on every other context
    const ForcedK<T> fk = m.forced ? forced_values<T>(c->p.tau, c->collision_param, c->collision_param2) : ForcedK<T>{};
    m.frc_hx = fk.hx; m.frc_hy = fk.hy;
    m.initial = 0;
    m.rho = m.ux = m.uy = nullptr; m.max_usq_bits = nullptr;
    return m;
}

// Dry run: the record of a sample of iteration t, with the rows ChoreoOp::samples says its kind reads.
inline int record_sample(lbm_ctx* c, int kind, int t) {
    ChoreoOp o;
    o.kind = kind; o.strip = o.r_strip = c->group_k; o.stream = 0; o.buf = c->cur; o.t = t;
    o.r0 = o.sample().lo; o.r1 = c->nyl + o.sample().hi;
    c->rec->ops.push_back(o);
    return LBM_OK;
}

// One sample of the running statistics (k_stats) at a force-output iteration t: buf[cur] = P_t. The snapshot it adds is the one
// do_macros takes from buf[cur ^ 1] once steps_done == t + 1. Queued on the compute stream behind join_comm, like the force kernel.
template <typename T>
int launch_stats(lbm_ctx* c, int t) {
    if (c->rec) { c->stats_n++; return record_sample(c, ChoreoOp::STATS, t); }
    StatsArgs<T> s;
    s.m = make_macro_args<T>(c, c->buf[c->cur], t);
    s.acc = c->d_stats; s.cells = (long)c->nx * c->nyl;
    dim3 grid((c->nx + 511) / 512, c->nyl), block(256);
    hipLaunchKernelGGL((k_stats<T>), grid, block, 0, c->stream, s);
    HIPCHK(hipGetLastError());
    c->stats_n++;
    return LBM_OK;
}

template <typename T>
int launch_forces(lbm_ctx* c, double* out, int t) {
    if (c->rec) return record_sample(c, ChoreoOp::FORCES, t);
    ForceArgs<T> f;
    f.cur = static_cast<const T*>(c->buf[c->cur]);
    f.plane = (long)c->plane; f.pitch = c->pitch; f.xoff = c->xoff;
    f.nx = c->nx; f.ny_loc = c->nyl; f.ny_glob = rows_glob(c); f.y_start = row_start(c);
    f.cyl_x = c->cyl_x; f.cyl_y = c->cyl_y; f.cyl_r = c->cyl_r; f.cyl_r2 = (double)(c->cyl_r * c->cyl_r);
    f.out = out; f.t = t; f.part = c->d_fpart;
    if (geom_masked(c)) {   // the mask's bounding box + 1 cell, within this strip's rows; large boxes in fixed chunks (k_forces)
        const HostMask& h = geom_mask(c);    // (periodic y: the box of the wrapped window, in the rows the kernels count)
        f.mv = c->mview;
        f.x0 = std::max(0, h.bx0 - 1);
        f.x1 = std::min(c->nx - 1, h.bx1 + 1);
        f.y0 = std::max(0, h.by0 - 1 - row_start(c));
        f.y1 = std::min(c->nyl - 1, h.by1 + 1 - row_start(c));
        if (h.bx1 < h.bx0) f.x1 = f.x0 - 1;    // no solid cell: no link
        const long ncell = (f.x1 >= f.x0 && f.y1 >= f.y0) ? (long)(f.x1 - f.x0 + 1) * (f.y1 - f.y0 + 1) : 0;
        const int nchunks = (int)std::max(1L, (ncell + FORCE_CHUNK - 1) / FORCE_CHUNK);
        hipLaunchKernelGGL((k_forces<T>), dim3(nchunks), dim3(1024), 0, c->stream, f);
        if (nchunks > 1) hipLaunchKernelGGL((k_forces_sum<T>), dim3(1), dim3(64), 0, c->stream, (const double*)c->d_fpart, nchunks, out, t);
        HIPCHK(hipGetLastError());
        return LBM_OK;
    }
    f.x0 = std::max(0, c->cyl_x - c->cyl_r - 1);
    f.x1 = std::min(c->nx - 1, c->cyl_x + c->cyl_r + 1);
    f.y0 = std::max(0, c->cyl_y - c->cyl_r - 1 - c->p.y_start);
    f.y1 = std::min(c->nyl - 1, c->cyl_y + c->cyl_r + 1 - c->p.y_start);
    hipLaunchKernelGGL((k_forces<T>), dim3(1), dim3(1024), 0, c->stream, f);
    HIPCHK(hipGetLastError());
    return LBM_OK;
}

// The per-body sample of iteration t (k_forces_bodies + k_forces_bodies_sum, lbm_set_body_labels): B rows (t, fx, fy) at `out`. Queued
// directly behind the force kernel on the compute stream: it reads the same rows of the same buffer, so the join that kernel sits
// behind covers it. One launch of one block per chunk of the table and one ordered sum, whatever the plan.
template <typename T>
int launch_body_forces(lbm_ctx* c, double* out, int t) {
    if (c->rec) return record_sample(c, ChoreoOp::BODIES, t);
    BodyForceArgs<T> a;
    a.cur = static_cast<const T*>(c->buf[c->cur]);
    a.plane = (long)c->plane; a.pitch = c->pitch; a.xoff = c->xoff; a.nx = c->nx;
    a.lab = c->d_labels; a.box = c->d_body_box; a.chunks = c->d_body_chunks; a.part = c->d_body_part;
    if (c->body_chunks > 0) hipLaunchKernelGGL((k_forces_bodies<T>), dim3(c->body_chunks), dim3(1024), 0, c->stream, a);
    hipLaunchKernelGGL((k_forces_bodies_sum<T>), dim3((c->body_n + 63) / 64), dim3(64), 0, c->stream, (const double*)c->d_body_part,
                       (const int*)c->d_body_first, c->body_n, out, t);
    HIPCHK(hipGetLastError());
    return LBM_OK;
}

// One frame (k_frame, lbm_frames_begin) of a force-output iteration t into the next free slot of the ring: buf[cur] = P_t, the snapshot
// that of launch_stats. Queued directly behind the force kernel on the compute stream, behind the same join. sample_outputs has
// checked that the ring has room.
template <typename T>
int launch_frame_sample(lbm_ctx* c, int t) {
    if (c->rec) return record_sample(c, ChoreoOp::FRAME, t);
    FrameArgs<T> f;
    f.m = make_macro_args<T>(c, c->buf[c->cur], t);
    f.k = c->frames_k; f.cnx = c->nx / c->frames_k; f.cny = c->nyl / c->frames_k;
    f.out = c->frames.next_slot();
    launch_frame<T>(f, c->stream);
    HIPCHK(hipGetLastError());
    c->frames.commit(t);
    return LBM_OK;
}

// One sample of the point probes (k_probes, lbm_probes_begin) of a force-output iteration t into the next free slot of the ring:
// buf[cur] = P_t, the snapshot that of launch_stats. Queued directly behind the force kernel (and the body, statistics and frame samples)
// on the compute stream, behind the same join. sample_outputs has checked that the ring has room.
template <typename T>
int launch_probe_sample(lbm_ctx* c, int t) {
    if (c->rec) return record_sample(c, ChoreoOp::PROBES, t);
    ProbeArgs<T> a;
    a.m = make_macro_args<T>(c, c->buf[c->cur], t);
    a.table = static_cast<const ProbeEntry*>(c->d_probe_table);
    a.n = c->probe_n;
    a.out = c->probes.next_slot();
    launch_probes<T>(a, c->stream);
    HIPCHK(hipGetLastError());
    c->probes.commit(t);
    return LBM_OK;
}

// The output point of a force-output iteration t (buf[cur] = P_t), the one place a sampler plugs into do_steps: every capacity check
// before anything is queued (a dry run has no frame or probe ring: nothing is launched), the join — the edge bands of the previous
// launch live on the side stream —, the force kernel and its log row, then the per-body rows, the statistics, the frame and the probes
// of iteration t, each directly behind it on the compute stream with no synchronisation. A counter advances once its launch is queued.
inline int join_comm(lbm_ctx* c);
template <typename T>
int sample_outputs(lbm_ctx* c, int t) {
    if (c->force_log.ix.full()) return fail(LBM_ERR_ARG, "force log full (%d rows): drain it", c->force_log.ix.cap);
    if (c->body_n > 0 && c->body_log.ix.full()) return fail(LBM_ERR_ARG, "body force log full (%d samples): drain it", c->body_log.ix.cap);
    if (c->frames_active && !c->rec && c->frames.ix.full()) return fail(LBM_ERR_ARG, "frame ring full (%d frames): drain it (lbm_drain_frames)", c->frames.ix.cap);
    if (c->probes_active && !c->rec && c->probes.ix.full()) return fail(LBM_ERR_ARG, "probe ring full (%d samples): drain it (lbm_drain_probes)", c->probes.ix.cap);
    int rc = join_comm(c);
    if (!rc) rc = launch_forces<T>(c, c->force_log.next_slot(), t);
    if (!rc) c->force_log.commit(t);
    if (!rc && c->body_n > 0) rc = launch_body_forces<T>(c, c->body_log.next_slot(), t);      // (a sample of the log at exactly the iterations of a force-log row)
    if (!rc && c->body_n > 0) c->body_log.commit(t);
    if (!rc && c->stats_active && t >= c->stats_from) rc = launch_stats<T>(c, t);
    if (!rc && c->frames_active) rc = launch_frame_sample<T>(c, t);
    if (!rc && c->probes_active) rc = launch_probe_sample<T>(c, t);
    return rc;
}

// What lbm_frames_begin and lbm_probes_begin share once the arguments are accepted: everything queued is waited for (a sample still in
// flight writes the ring this call replaces), the old ring goes and one of `capacity` slots of `per` elements takes its place.
// LBM_ERR_ALLOC: no device memory, and no ring (the caller says which); any other error: nothing was touched.
template <typename E>
int replace_ring(lbm_ctx* c, DeviceRing<E>& ring, size_t per, int capacity) {
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (ring.alloc(per, capacity, true) != hipSuccess) { (void)hipGetLastError(); return LBM_ERR_ALLOC; }
    return LBM_OK;
}
