"""ctypes view of include/lbm_hip.h (liblbm_hip.so). No numerics here; every call goes to the HIP library."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("LBM_HIP_LIBRARY") or os.path.join(HERE, "csrc", "liblbm_hip.so")   # (override: diagnostic builds)


class LbmError(RuntimeError):
    pass


class Params(C.Structure):
    """struct lbm_params (include/lbm_hip.h) == the physics fields of LBM::SimulationParams + the strip."""
    _fields_ = [("tau", C.c_double), ("inlet_velocity", C.c_double), ("nx", C.c_int), ("ny", C.c_int),
                ("cylinder_x", C.c_double), ("cylinder_y", C.c_double), ("cylinder_radius", C.c_double),
                ("y_start", C.c_int), ("local_ny", C.c_int), ("precision", C.c_int),
                ("force_log_capacity", C.c_int)]


class ForceRow(C.Structure):
    _fields_ = [("timestep", C.c_int), ("fx", C.c_double), ("fy", C.c_double)]


class BodyForceRow(C.Structure):
    _fields_ = [("timestep", C.c_int), ("body", C.c_int), ("fx", C.c_double), ("fy", C.c_double)]


class CkptHead(C.Structure):
    """struct lbm_ckpt_head (include/lbm_hip.h): what the head of a checkpoint says about a run."""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("y_start", C.c_int), ("local_ny", C.c_int), ("precision", C.c_int), ("steps_done", C.c_int),
                ("tau", C.c_double), ("inlet_velocity", C.c_double), ("cylinder_x", C.c_double), ("cylinder_y", C.c_double),
                ("cylinder_radius", C.c_double),
                ("has_mask", C.c_int), ("has_profile", C.c_int), ("collision", C.c_int), ("has_walls", C.c_int), ("has_sched", C.c_int),
                ("mask_digest", C.c_ulonglong), ("profile_digest", C.c_ulonglong), ("sched_digest", C.c_ulonglong),
                ("collision_param", C.c_double * 2), ("walls", C.c_double * 4), ("has_ports", C.c_int), ("ports", C.c_double * 4),
                ("has_periodic_y", C.c_int)]


CKPT_HEAD_MAX = 184                                            # LBM_CKPT_HEAD_MAX

_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Loads liblbm_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise LbmError(f"{_LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        L = C.CDLL(_LIB_PATH)
        dp = C.POINTER(C.c_double)
        vp = C.c_void_p
        L.lbm_last_error.restype = C.c_char_p
        L.lbm_device_count.restype = C.c_int
        L.lbm_create.argtypes = [C.POINTER(Params), C.c_int, C.POINTER(vp)]
        L.lbm_destroy.argtypes = [vp]; L.lbm_destroy.restype = None
        L.lbm_initialise.argtypes = [vp, C.POINTER(C.c_int)]
        L.lbm_step.argtypes = [vp, C.c_int, C.c_int]
        L.lbm_sync.argtypes = [vp]
        L.lbm_steps_done.argtypes = [vp]
        L.lbm_first_unstable_step.argtypes = [vp, C.POINTER(C.c_int)]
        L.lbm_get_forces.argtypes = [vp, dp, dp]
        L.lbm_drain_force_log.argtypes = [vp, C.POINTER(ForceRow), C.c_int]
        L.lbm_get_macros.argtypes = [vp, dp, dp, dp]
        L.lbm_max_velocity_sq.argtypes = [vp, dp]
        L.lbm_stats_begin.argtypes = [vp, C.c_int]
        L.lbm_stats_end.argtypes = [vp]
        L.lbm_stats_samples.argtypes = [vp]
        L.lbm_get_stat_sums.argtypes = [vp, dp]
        L.lbm_stats_restore.argtypes = [vp, dp, C.c_int]
        L.lbm_frames_begin.argtypes = [vp, C.c_int, C.c_int]
        L.lbm_frames_end.argtypes = [vp]
        L.lbm_frames_pending.argtypes = [vp]
        L.lbm_drain_frames.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]
        L.lbm_probes_begin.argtypes = [vp, dp, C.c_int, C.c_int]
        L.lbm_probes_end.argtypes = [vp]
        L.lbm_probes_count.argtypes = [vp]
        L.lbm_probes_pending.argtypes = [vp]
        L.lbm_drain_probes.argtypes = [vp, C.POINTER(C.c_int), dp, C.c_int]
        L.lbm_debug_probe_table.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), dp, C.POINTER(C.c_int)]
        L.lbm_get_populations.argtypes = [vp, C.c_int, dp]
        L.lbm_set_f_current.argtypes = [vp, dp]
        L.lbm_get_solid.argtypes = [vp, C.POINTER(C.c_ubyte)]
        L.lbm_set_solid_mask.argtypes = [vp, C.POINTER(C.c_ubyte), C.c_int, C.c_int]
        L.lbm_set_body_labels.argtypes = [vp, C.POINTER(C.c_ubyte), C.c_int, C.c_int]
        L.lbm_body_count.argtypes = [vp]
        L.lbm_get_body_forces.argtypes = [vp, dp]
        L.lbm_drain_body_force_log.argtypes = [vp, C.POINTER(BodyForceRow), C.c_int]
        L.lbm_debug_body_chunks.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                            C.POINTER(C.c_long), C.c_int, C.POINTER(C.c_int)]
        L.lbm_set_inlet_profile.argtypes = [vp, dp, C.c_int]
        L.lbm_set_smagorinsky.argtypes = [vp, C.c_double]
        L.lbm_set_trt.argtypes = [vp, C.c_double]
        L.lbm_set_forcing.argtypes = [vp, C.c_double, C.c_double]
        L.lbm_get_forcing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.lbm_set_mrt.argtypes = [vp, C.c_double, C.c_double]
        L.lbm_get_mrt.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.lbm_set_sponge.argtypes = [vp, C.c_int, C.c_double]
        L.lbm_get_sponge.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.lbm_get_sponge_rate.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
        L.lbm_debug_sponge_rates.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, dp, dp]
        L.lbm_debug_collision_args.argtypes = [C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, dp, C.c_int]
        L.lbm_set_wall.argtypes = [vp, C.c_int, C.c_int, C.c_double]
        L.lbm_get_wall.argtypes = [vp, C.c_int, C.POINTER(C.c_int), dp]
        L.lbm_debug_wall_rule.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, dp, dp]
        L.lbm_set_port.argtypes = [vp, C.c_int, C.c_int, C.c_double]
        L.lbm_get_port.argtypes = [vp, C.c_int, C.POINTER(C.c_int), dp]
        L.lbm_set_periodic_y.argtypes = [vp, C.c_int]
        L.lbm_get_periodic_y.argtypes = [vp]
        L.lbm_debug_port_rule.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, dp, dp, dp, dp]
        L.lbm_set_inlet_schedule.argtypes = [vp, dp, C.c_int, C.c_int]
        L.lbm_inlet_schedule_length.argtypes = [vp]
        L.lbm_get_inlet_scale.argtypes = [vp, C.c_int, dp]
        L.lbm_debug_inlet_scale.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, dp]
        ip = C.POINTER(C.c_int)
        L.lbm_debug_geometry.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_ulonglong), C.c_long,
                                         ip, C.c_long, ip, C.c_int, ip]
        L.lbm_debug_ring.argtypes = [C.c_int, ip, C.c_int, ip]
        L.lbm_comm_unique_id.argtypes = [vp]
        L.lbm_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
        L.lbm_comm_allreduce.argtypes = [vp, dp, C.c_int, C.c_int]
        pp = C.POINTER(vp)
        L.lbm_group_link.argtypes = [pp, C.c_int, C.c_int]
        L.lbm_group_initialise.argtypes = [pp, C.c_int, C.POINTER(C.c_int)]
        L.lbm_group_step.argtypes = [pp, C.c_int, C.c_int, C.c_int]
        L.lbm_group_refresh_halos.argtypes = [pp, C.c_int]
        L.lbm_group_first_unstable_step.argtypes = [pp, C.c_int, ip]
        L.lbm_group_max_velocity_sq.argtypes = [pp, C.c_int, dp]
        L.lbm_group_get_forces.argtypes = [pp, C.c_int, dp, dp]
        L.lbm_group_drain_force_log.argtypes = [pp, C.c_int, C.POINTER(ForceRow), C.c_int]
        L.lbm_group_get_body_forces.argtypes = [pp, C.c_int, dp]
        L.lbm_group_drain_body_force_log.argtypes = [pp, C.c_int, C.POINTER(BodyForceRow), C.c_int]
        L.lbm_group_get_macros.argtypes = [pp, C.c_int, dp, dp, dp]
        L.lbm_group_get_populations.argtypes = [pp, C.c_int, C.c_int, dp]
        L.lbm_group_stats_samples.argtypes = [pp, C.c_int]
        L.lbm_group_get_stat_sums.argtypes = [pp, C.c_int, dp]
        L.lbm_group_stats_restore.argtypes = [pp, C.c_int, dp, C.c_int]
        L.lbm_group_frames_pending.argtypes = [pp, C.c_int]
        L.lbm_group_probes_pending.argtypes = [pp, C.c_int]
        L.lbm_group_drain_frames.argtypes = [pp, C.c_int, ip, C.POINTER(C.c_float), C.c_int]
        L.lbm_group_drain_probes.argtypes = [pp, C.c_int, ip, dp, C.c_int]
        L.lbm_debug_gather.argtypes = [C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, pp, vp]
        L.lbm_halo_export.argtypes = [vp, dp, dp]
        L.lbm_halo_import.argtypes = [vp, dp, dp]
        L.lbm_set_option.argtypes = [vp, C.c_char_p, C.c_long]
        L.lbm_save_state.argtypes = [vp, C.c_char_p]
        L.lbm_load_state.argtypes = [vp, C.c_char_p]
        L.lbm_debug_ckpt_save.argtypes = [C.POINTER(CkptHead), C.POINTER(C.c_ubyte), dp, dp, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.lbm_debug_ckpt_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(CkptHead), C.c_char_p, ip]
        L.lbm_last_step_kernel_ms.argtypes = [vp, dp]
        L.lbm_last_step_stats.argtypes = [vp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.lbm_last_step_dispatches.argtypes = [vp]
        L.lbm_graph_replays.restype = C.c_long; L.lbm_graph_replays.argtypes = [vp]
        L.lbm_kernel_name.argtypes = [vp]; L.lbm_kernel_name.restype = C.c_char_p
        L.lbm_plan.argtypes = [vp]; L.lbm_plan.restype = C.c_char_p
        L.lbm_plan_options.argtypes = [vp]; L.lbm_plan_options.restype = C.c_char_p
        L.lbm_build_id.restype = C.c_char_p
        L.lbm_runtime_versions.argtypes = [C.POINTER(C.c_int)] * 3
        L.lbm_strip_schedule.argtypes = [vp]; L.lbm_strip_schedule.restype = C.c_char_p
        L.lbm_device_memory.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        _lib = L
    return _lib


def device_count():
    return lib().lbm_device_count()


def runtime_versions():
    """{'rccl': .., 'hip_runtime': .., 'hip_driver': ..} as bound by THIS process (ncclGetVersion etc.)."""
    r, h, d = C.c_int(), C.c_int(), C.c_int()
    if lib().lbm_runtime_versions(C.byref(r), C.byref(h), C.byref(d)) < 0:
        raise LbmError(lib().lbm_last_error().decode())
    return {"rccl": r.value, "hip_runtime": h.value, "hip_driver": d.value}


def device_memory(device=0):
    """(free, total) bytes of a device (hipMemGetInfo)."""
    f, t = C.c_ulonglong(), C.c_ulonglong()
    if lib().lbm_device_memory(device, C.byref(f), C.byref(t)) < 0:
        raise LbmError(lib().lbm_last_error().decode())
    return f.value, t.value


def build_id():
    """Source hash the loaded library was compiled from (lbm_build_id)."""
    return lib().lbm_build_id().decode()


def _mask_bytes(solid, nx, ny):
    """A bool / integer (ny, nx) array as the contiguous uint8 0/1 array lbm_set_solid_mask reads."""
    m = np.asarray(solid)
    if m.shape != (ny, nx):
        raise ValueError(f"solid mask has shape {m.shape}, the domain is (ny, nx) = {(ny, nx)}")
    if not (m.dtype == np.bool_ or np.issubdtype(m.dtype, np.integer)):
        raise TypeError(f"solid mask must be bool or uint8, not {m.dtype}")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def debug_geometry(solid, y_start=0, local_ny=0, boxes=()):
    """lbm_debug_geometry (no device): the packing lbm_set_solid_mask makes for one strip of a global (ny, nx) mask.
    Returns (dims, bits [rows, words] uint64, sat [nby+1, nbx+1] int32, near [len(boxes)]) with dims = {y0, rows, words, nbx, nby,
    bx0, bx1, by0, by1}; boxes = [(x0, x1, y0, y1)] global inclusive, near[k] = the kernels' near-solid query for box k."""
    L = lib()
    ny, nx = np.shape(solid)
    m = _mask_bytes(solid, nx, ny)
    local_ny = local_ny if local_ny > 0 else ny - y_start
    dims = (C.c_int * 9)()
    ub = C.POINTER(C.c_ubyte)
    if L.lbm_debug_geometry(m.ctypes.data_as(ub), nx, ny, y_start, local_ny, dims, None, 0, None, 0, None, 0, None) < 0:
        raise LbmError(L.lbm_last_error().decode())
    d = dict(zip(("y0", "rows", "words", "nbx", "nby", "bx0", "bx1", "by0", "by1"), list(dims)))
    bits = np.zeros((d["rows"], d["words"]), dtype=np.uint64)
    sat = np.zeros((d["nby"] + 1, d["nbx"] + 1), dtype=np.int32)
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
    near = np.zeros(len(b), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    rc = L.lbm_debug_geometry(m.ctypes.data_as(ub), nx, ny, y_start, local_ny, dims, bits.ctypes.data_as(C.POINTER(C.c_ulonglong)), bits.size,
                              sat.ctypes.data_as(ip), sat.size, b.ctypes.data_as(ip), len(b), near.ctypes.data_as(ip))
    if rc < 0:
        raise LbmError(L.lbm_last_error().decode())
    return d, bits, sat, near


def debug_ring(capacity, ops):
    """lbm_debug_ring (no device): the index arithmetic of the sample rings (body-force log, frames, probes) on a ring of `capacity` slots.
    ops: -1 pushes, m >= 0 takes up to m of the oldest. Returns (one triple per operation, samples pending at the end): a push gives
    (slot, -1, -1), or (-1, -1, -1) on a full ring; a take gives (start, n1, n2): slots [start, start + n1), then [0, n2)."""
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    out = np.zeros((len(ops), 3), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib().lbm_debug_ring(capacity, ops.ctypes.data_as(ip), len(ops), out.ctypes.data_as(ip))
    if rc < 0:
        raise LbmError(lib().lbm_last_error().decode())
    return out, rc


def debug_gather(what, bounds, nx, ny, parts, whole, k=1, planes=1):
    """lbm_debug_gather (no device): the rules of the group gathers on one C-contiguous array per strip, bounds = [(y_start, rows)].
    what: "stack" / "stack_f32" (parts -> whole at row y_start / k), "unstack" (whole -> parts), "populations" (the ghost-row rule),
    "sum" (the strips' nx * planes doubles added in strip order into whole). Writes whole (unstack: the parts) in place."""
    b = np.ascontiguousarray(bounds, dtype=np.int32).reshape(-1, 2)
    ptrs = (C.c_void_p * len(parts))(*[p.ctypes.data for p in parts])
    code = {"stack": 0, "unstack": 1, "stack_f32": 2, "populations": 3, "sum": 4}[what]
    if lib().lbm_debug_gather(code, len(parts), b.ctypes.data_as(C.POINTER(C.c_int)), nx, ny, k, planes, ptrs, whole.ctypes.data) < 0:
        raise LbmError(lib().lbm_last_error().decode())


def debug_ckpt_save(head, mask=None, profile=None, schedule=None):
    """lbm_debug_ckpt_save (no device): the bytes of the head lbm_save_state writes for a context that `head` (a CkptHead) describes.
    mask ((ny, nx)), profile ((ny,)) or schedule (inlet_schedule= form): that field is marked present in `head` and its digest is formed
    from the data as the setter forms it, and left in `head`."""
    m = _mask_bytes(mask, head.nx, head.ny) if mask is not None else None
    u = np.ascontiguousarray(profile, dtype=np.float64) if profile is not None else None
    if u is not None and u.shape != (head.ny,):
        raise ValueError(f"an inlet profile has one velocity per row: shape {u.shape}, the domain has {head.ny} rows")
    s, mode = _schedule(schedule) if schedule is not None else (None, 0)
    out = C.create_string_buffer(CKPT_HEAD_MAX)
    n = lib().lbm_debug_ckpt_save(C.byref(head), m.ctypes.data_as(C.POINTER(C.c_ubyte)) if m is not None else None, _dp(u), _dp(s),
                                  s.size if s is not None else 0, mode, out, CKPT_HEAD_MAX)
    if n < 0:
        raise LbmError(f"lbm_hip error {n}: {lib().lbm_last_error().decode()}")
    return out.raw[:n]


def debug_ckpt_load(data, head, path="x.ckpt"):
    """lbm_debug_ckpt_load (no device): what lbm_load_state decides about a file `path` that begins with the bytes `data`, on a context that
    `head` (a CkptHead) describes: the bytes of the file's head, behind which the populations stand; LbmError with lbm_load_state's text."""
    used = C.c_int()
    rc = lib().lbm_debug_ckpt_load(bytes(data), len(data), C.byref(head), path.encode(), C.byref(used))
    if rc < 0:
        raise LbmError(lib().lbm_last_error().decode())
    return used.value


def _label_bytes(labels, nx, ny):
    """An integer (ny, nx) array of body numbers 0..255 as the contiguous uint8 array lbm_set_body_labels reads."""
    m = np.asarray(labels)
    if m.shape != (ny, nx):
        raise ValueError(f"body labels have shape {m.shape}, the domain is (ny, nx) = {(ny, nx)}")
    if not np.issubdtype(m.dtype, np.integer):
        raise TypeError(f"body labels must be integers, not {m.dtype}")
    if m.size and (m.min() < 0 or m.max() > 255):
        raise ValueError("body labels must lie in 0..255")
    return np.ascontiguousarray(m, dtype=np.uint8)


def debug_body_chunks(labels, y_start=0, local_ny=0):
    """lbm_debug_body_chunks (no device): what lbm_set_body_labels derives for one strip of a global (ny, nx) label array.
    Returns (B, boxes [B, 4] int32 = x0, x1, y0, y1 inclusive in (x, local y), {0, -1, 0, -1} where empty,
    chunks [n, 3] int64 = body, first cell of the box, cells)."""
    L = lib()
    ny, nx = np.shape(labels)
    m = _label_bytes(labels, nx, ny)
    local_ny = local_ny if local_ny > 0 else ny - y_start
    ub = C.POINTER(C.c_ubyte)
    n = C.c_int()
    B = L.lbm_debug_body_chunks(m.ctypes.data_as(ub), nx, ny, y_start, local_ny, None, 0, None, 0, C.byref(n))
    if B < 0:
        raise LbmError(L.lbm_last_error().decode())
    boxes = np.zeros((B, 4), dtype=np.int32)
    chunks = np.zeros((n.value, 3), dtype=np.int64)
    rc = L.lbm_debug_body_chunks(m.ctypes.data_as(ub), nx, ny, y_start, local_ny, boxes.ctypes.data_as(C.POINTER(C.c_int)), B,
                                 chunks.ctypes.data_as(C.POINTER(C.c_long)), n.value, None)
    if rc < 0:
        raise LbmError(L.lbm_last_error().decode())
    return B, boxes, chunks


def parabolic_profile(ny, mean):
    """The inlet profile of lbm_solver --inlet-profile parabolic (host/lbm/inlet.hpp, operation by operation): the Poiseuille
    shape s(1-s), s = (y + 0.5)/ny, scaled so that its mean over the ny rows is `mean`. float64 [ny], row 0 (bottom) first."""
    return scale_inlet_profile(parabolic_shape(ny), mean)


def parabolic_shape(ny):
    s = (np.arange(ny, dtype=np.float64) + 0.5) / ny
    return s * (1.0 - s)


def scale_inlet_profile(shape, mean):
    """u[y] = shape[y] * (mean / (sum of the shape, rows in order, / ny)), as lbm_solver scales a profile file's shape."""
    shape = np.asarray(shape, dtype=np.float64)
    total = 0.0
    for v in shape.tolist():   # sequential, in row order (numpy's pairwise sum would round differently)
        total += v
    shape_mean = total / len(shape)
    if not (np.isfinite(shape_mean) and shape_mean > 0.0):
        raise ValueError("the mean of an inlet profile's shape must be positive")
    u = shape * (mean / shape_mean)
    if not np.all(u < 1.0):
        raise ValueError("inlet velocities must stay below 1")
    return u


INLET_MODES = {"hold": 0, "repeat": 1}                         # LBM_INLET_HOLD / LBM_INLET_REPEAT
INLET_SCHEDULE_MAX = 1048576                                   # LBM_INLET_SCHEDULE_MAX


def cosine_ramp(n):
    """The schedule of lbm_solver --inlet-ramp N (host/lbm/inlet.hpp cosine_ramp, operation by operation): N + 1 factors
    0.5 * (1 - cos(pi * k / N)), from 0 to 1; used with "hold"."""
    n = int(n)
    if n < 1:
        raise ValueError("a ramp takes at least one step")
    k = np.arange(n + 1, dtype=np.float64)
    return 0.5 * (1.0 - np.cos(np.pi * k / n))


def sine_pulse(amplitude, period):
    """The schedule of lbm_solver --inlet-pulse A:P (host/lbm/inlet.hpp sine_pulse, operation by operation): P factors
    1 + A * sin(2 * pi * k / P); used with "repeat"."""
    period = int(period)
    if period < 1:
        raise ValueError("a pulse has a period of at least one iteration")
    k = np.arange(period, dtype=np.float64)
    return 1.0 + float(amplitude) * np.sin(2.0 * np.pi * k / period)


def sponge_tau(nx, tau, width, tau_end):
    """The relaxation time of every column under lbm_set_sponge(width, tau_end), float64 [nx], operation by operation as the library forms
    it: tau up to column x0 = nx - 1 - width, then tau + (tau_end - tau) * (s * s) with s = (x - x0) / width. The kernels relax column x
    with the rate (1 / sponge_tau)[x] cast once to their element type (Context.sponge_rate). width 0: tau everywhere."""
    nx, width, tau, tau_end = int(nx), int(width), float(tau), float(tau_end)
    if nx < 1 or width < 0 or width > nx - 1:
        raise ValueError("a sponge of %d columns does not fit %d columns (0 .. nx - 1; column 0 keeps tau)" % (width, nx))
    t = np.full(nx, tau, dtype=np.float64)
    if width > 0:
        x0 = nx - 1 - width
        s = np.arange(1, width + 1, dtype=np.float64) / np.float64(width)
        t[x0 + 1:] = tau + (tau_end - tau) * (s * s)
    return t


def debug_sponge_rates(nx, tau, precision, width, tau_end):
    """lbm_debug_sponge_rates (no device): lbm_set_sponge on a context of nx columns, then what lbm_get_sponge and lbm_get_sponge_rate
    report: ((width, tau_end), float64 [nx] rates). precision: "f64" / "f32". Raises LbmError with the setter's text if it refuses."""
    pair, rates = np.zeros(2, dtype=np.float64), np.zeros(int(nx), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    rc = lib().lbm_debug_sponge_rates(int(nx), float(tau), 1 if precision in ("f32", 1) else 0, int(width), float(tau_end),
                                      pair.ctypes.data_as(dp), rates.ctypes.data_as(dp))
    if rc != 0:
        raise LbmError(lib().lbm_last_error().decode())
    return (int(pair[0]), float(pair[1])), rates


def debug_collision_args(tau, precision, setter, v1=0.0, v2=0.0):
    """lbm_debug_collision_args (no device): the launch-uniform values of one collision model as a launch carries them. setter: -1 plain
    BGK, 0 lbm_set_smagorinsky(v1), 1 lbm_set_trt(v1), 2 lbm_set_forcing(v1, v2), 3 lbm_set_mrt(v1, v2), 6 lbm_set_sponge(int(v1), v2).
    Returns (named values in the model's order, the seven shared slots), both float64 arrays. precision: "f64" / "f32". Raises
    LbmError with the setter's text if it refuses."""
    out = np.zeros(16, dtype=np.float64)
    n = lib().lbm_debug_collision_args(float(tau), 1 if precision in ("f32", 1) else 0, int(setter), float(v1), float(v2),
                                       out.ctypes.data_as(C.POINTER(C.c_double)), len(out))
    if n < 0:
        raise LbmError(lib().lbm_last_error().decode())
    return out[:n].copy(), out[n:n + 7].copy()


def _schedule(spec):
    """The inlet_schedule= keyword as (float64 table, mode number): a table (hold) or a pair (table, "hold" | "repeat" | 0 | 1)."""
    mode = 0
    if isinstance(spec, tuple) and len(spec) == 2 and (isinstance(spec[1], str) or np.ndim(spec[0]) > 0):
        spec, m = spec
        if isinstance(m, str):
            if m not in INLET_MODES:
                raise ValueError(f"unknown inlet schedule mode {m!r}: one of {sorted(INLET_MODES)}")
            mode = INLET_MODES[m]
        else:
            mode = int(m)
    return np.ascontiguousarray(np.atleast_1d(spec), dtype=np.float64), mode


def debug_inlet_scale(s, mode, t, precision="f64"):
    """lbm_debug_inlet_scale (no device): the factor (double)(T)s(t) the schedule (s, mode) gives each iteration of `t`, through the
    index function the kernels call."""
    a, m = _schedule((np.asarray(s, dtype=np.float64), mode))
    tt = np.ascontiguousarray(np.atleast_1d(t), dtype=np.int32)
    out = np.empty(tt.size, dtype=np.float64)
    rc = lib().lbm_debug_inlet_scale(_dp(a), a.size, m, {"f64": 0, "f32": 1}[precision], tt.ctypes.data_as(C.POINTER(C.c_int)),
                                     tt.size, _dp(out))
    if rc < 0:
        raise LbmError(f"lbm_hip error {rc}: {lib().lbm_last_error().decode()}")
    return out


WALL_SIDES = {"south": 0, "north": 1}                          # LBM_WALL_SOUTH / LBM_WALL_NORTH
WALL_KINDS = {"no-slip": 0, "free-slip": 1, "moving": 2}       # LBM_WALL_NOSLIP / LBM_WALL_FREESLIP / LBM_WALL_MOVING
_WALL_NAMES = {v: k for k, v in WALL_KINDS.items()}


def _wall_code(table, what, v):
    """A side / kind given by name or by its LBM_WALL_* number -> the number (numbers pass through: the library checks their range)."""
    if isinstance(v, str):
        if v not in table:
            raise ValueError(f"unknown wall {what} {v!r}: one of {sorted(table)}")
        return table[v]
    return int(v)


def _wall_pair(walls):
    """The walls= keyword as ((south kind, south velocity), (north kind, north velocity)): "free-slip" / "no-slip" for both walls, or a
    pair (south, north) whose entries are "no-slip", "free-slip" or ("moving", u_w)."""
    def one(w):
        if isinstance(w, str):
            if w == "moving":
                raise ValueError('a moving wall is given as ("moving", u_w)')
            return _wall_code(WALL_KINDS, "kind", w), 0.0
        kind, u = w
        return _wall_code(WALL_KINDS, "kind", kind), float(u)
    if isinstance(walls, str):
        return one(walls), one(walls)
    south, north = walls
    return one(south), one(north)


def debug_wall_rule(side, kind, velocity, f9, precision="f64"):
    """lbm_debug_wall_rule (no device): the kernels' wall rule on ONE cell. f9: the nine pulled populations; they are cast to the element
    type, the rule of wall `side` ("south" / "north") with `kind` and `velocity` is applied, and the nine results come back as float64."""
    a = np.ascontiguousarray(f9, dtype=np.float64)
    if a.shape != (9,):
        raise ValueError(f"a cell has nine populations, not shape {a.shape}")
    out = np.empty(9, dtype=np.float64)
    rc = lib().lbm_debug_wall_rule(_wall_code(WALL_SIDES, "side", side), _wall_code(WALL_KINDS, "kind", kind), float(velocity),
                                   {"f64": 0, "f32": 1}[precision], _dp(a), _dp(out))
    if rc < 0:
        raise LbmError(f"lbm_hip error {rc}: {lib().lbm_last_error().decode()}")
    return out


PORT_SIDES = {"west": 0, "east": 1}                            # LBM_PORT_WEST / LBM_PORT_EAST
PORT_KINDS = {"velocity": 0, "pressure": 1}                    # LBM_PORT_VELOCITY / LBM_PORT_PRESSURE
_PORT_NAMES = {v: k for k, v in PORT_KINDS.items()}
PORT_DEFAULTS = ((0, 0.0), (1, 1.0))                           # west (velocity, 0), east (pressure, 1): the reference's pair


def _port_code(table, what, v):
    """A side / kind given by name or by its LBM_PORT_* number -> the number (numbers pass through: the library checks their range)."""
    if isinstance(v, str):
        if v not in table:
            raise ValueError(f"unknown port {what} {v!r}: one of {sorted(table)}")
        return table[v]
    return int(v)


def _port_pair(ports):
    """The ports= keyword as ((west kind, west value), (east kind, east value)): a pair (west, east) with west "velocity" or
    ("pressure", rho) and east ("pressure", rho) or ("velocity", u); None in either place: that port's default."""
    west, east = ports

    def one(p, default, is_west):
        if p is None:
            return default
        if isinstance(p, str):             # the bare name: the west velocity port alone, which is given no value here
            if p != "velocity" or not is_west:
                raise ValueError(f'a port is "velocity" (west only), ("pressure", rho) or ("velocity", u) (east only), not {p!r}'
                                 f' in the {"west" if is_west else "east"} place')
            return PORT_KINDS["velocity"], 0.0
        kind, v = p
        return _port_code(PORT_KINDS, "kind", kind), float(v)
    return one(west, PORT_DEFAULTS[0], True), one(east, PORT_DEFAULTS[1], False)


def debug_port_rule(side, kind, value, f9, u_in=0.0, precision="f64"):
    """lbm_debug_port_rule (no device): the kernels' port rule on ONE cell. f9: the nine populations after the pull and the wall rule; they
    are cast to the element type, the rule of port `side` ("west" / "east") with `kind` ("velocity" / "pressure") and `value` is applied
    (a west velocity port is given u_in), and (the nine results, rho, u) come back as float64."""
    a = np.ascontiguousarray(f9, dtype=np.float64)
    if a.shape != (9,):
        raise ValueError(f"a cell has nine populations, not shape {a.shape}")
    out = np.empty(9, dtype=np.float64)
    rho, u = C.c_double(), C.c_double()
    rc = lib().lbm_debug_port_rule(_port_code(PORT_SIDES, "side", side), _port_code(PORT_KINDS, "kind", kind), float(value), float(u_in),
                                   {"f64": 0, "f32": 1}[precision], _dp(a), _dp(out), C.byref(rho), C.byref(u))
    if rc < 0:
        raise LbmError(f"lbm_hip error {rc}: {lib().lbm_last_error().decode()}")
    return out, rho.value, u.value


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _stats_from_sums(sums, n):
    """The time averages of n samples from the six sums (rho, ux, uy, ux*ux, uy*uy, ux*uy): the means and the Reynolds stresses
    <u'u'> = S_uu / n - mean(u)^2, <v'v'>, <u'v'> (host arithmetic on the caller's side of the interface: include/lbm_hip.h)."""
    if n <= 0:
        raise LbmError("no statistics sample has been taken yet")
    rho, ux, uy = sums[0] / n, sums[1] / n, sums[2] / n
    return {"n": n, "rho": rho, "ux": ux, "uy": uy,
            "uxux": sums[3] / n - ux * ux, "uyuy": sums[4] / n - uy * uy, "uxuy": sums[5] / n - ux * uy}


def _probe_points(xy):
    """(n, 2) float64, C-contiguous: the probe points as lbm_probes_begin takes them."""
    a = np.ascontiguousarray(xy, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"probe points must have shape (n, 2), not {a.shape}")
    return a


class Context:
    """One strip of the lattice on one GPU (struct lbm_ctx). solid: optional bool / uint8 (ny, nx) array of the WHOLE domain, row
    y = 0 first, nonzero = solid (lbm_set_solid_mask): the obstacle geometry in place of the cylinder_* disc. inlet_profile: optional
    float64 [ny] of absolute inlet x-velocities of the WHOLE domain, row y = 0 first (lbm_set_inlet_profile), in place of the
    uniform inlet_velocity (see parabolic_profile). smagorinsky: optional constant Cs of a Smagorinsky LES collision
    (lbm_set_smagorinsky) in place of plain BGK; 0 / None: BGK. trt_magic: optional magic parameter of a two-relaxation-time
    collision (lbm_set_trt; 1/4 most stable, 3/16 most accurate at walls) in place of plain BGK; 0 / None: BGK; not with smagorinsky.
    bodies: optional integer (ny, nx) array of body numbers of the WHOLE
    domain (0 fluid, 1..255; lbm_set_body_labels): the geometry of solid=(bodies != 0) plus forces per body (body_forces,
    drain_body_force_log); not together with solid. frames: optional stride k of coarsened flow frames (lbm_frames_begin with the
    default capacity at the end of initialise(); see frames_begin). probes: optional (n, 2) array of probe points (x, y) in GLOBAL lattice
    coordinates (lbm_probes_begin with a ring of probe_capacity samples at the end of initialise(); see probes_begin). walls: optional
    kinds of the bottom and top walls (lbm_set_wall) in place of the two no-slip walls: "free-slip" (both), or a pair (south, north) whose
    entries are "no-slip", "free-slip" or ("moving", u_w) with the wall's tangential velocity u_w. inlet_schedule: optional table of
    scale factors of the inflow, one per iteration (lbm_set_inlet_schedule): a table holds its last entry for ever, a pair
    (table, "repeat") is periodic (see cosine_ramp, sine_pulse). forcing: optional pair (fx, fy), a uniform driving force density in
    lattice units on every fluid cell (lbm_set_forcing, Guo's scheme on BGK); (0, 0) / None: none; not with smagorinsky or trt_magic.
    mrt: optional pair (bulk_rate, magic) of a multiple-relaxation-time collision (lbm_set_mrt): TRT with that magic parameter whose
    bulk rate, in (0, 2), is free of tau (1/tau: TRT; lower: more bulk viscosity); bulk_rate 0 / None: BGK; not with smagorinsky,
    trt_magic or forcing.
    sponge: optional pair (width, tau_end) of an outlet sponge zone (lbm_set_sponge): over the last `width` columns the relaxation time
    rises from tau to tau_end (sponge_tau), so that what reaches the east port is diffused before it reflects; width 0 / None: none; not
    with smagorinsky, trt_magic, forcing or mrt.
    ports: optional pair (west, east) of the two open ends (lbm_set_port) in place of the velocity inlet and the pressure outlet with
    rho = 1: west "velocity" or ("pressure", rho), east ("pressure", rho) or ("velocity", u); None in either place: that port's default.
    A west pressure port takes neither inlet_profile nor inlet_schedule (initialise() fails). periodic_y: True makes the top and bottom
    boundaries periodic (lbm_set_periodic_y): row -1 is row ny - 1, no wall rule runs; not with walls other than no-slip, nor with bodies
    that touch row 0 or ny - 1 (initialise() fails)."""

    def __init__(self, nx, ny, tau=0.6, inlet_velocity=0.01333, cylinder_x=0.2, cylinder_y=0.5,
                 cylinder_radius=0.05, y_start=0, local_ny=0, precision="f64", device=0, force_log_capacity=0,
                 options=None, solid=None, inlet_profile=None, smagorinsky=None, bodies=None, frames=None, trt_magic=None,
                 probes=None, probe_capacity=None, walls=None, inlet_schedule=None, forcing=None, ports=None, periodic_y=False, mrt=None,
                 sponge=None):
        if solid is not None and bodies is not None:
            raise LbmError("solid= and bodies= exclude each other: the body labels are the geometry (solid where nonzero)")
        self.L = lib()
        self.params = Params(tau, inlet_velocity, nx, ny, cylinder_x, cylinder_y, cylinder_radius, y_start,
                             local_ny, {"f64": 0, "f32": 1}[precision], force_log_capacity)
        self.nx, self.ny = nx, ny
        self.y_start = y_start
        self.local_ny = local_ny if local_ny > 0 else ny - y_start
        self.h = C.c_void_p()
        self._chk(self.L.lbm_create(C.byref(self.params), device, C.byref(self.h)))
        self.solid_count = None
        self._frames_k = 0
        self._probes_kw = None if probes is None else (_probe_points(probes), probe_capacity)
        for k, v in (options or {}).items():
            self.set_option(k, v)
        if solid is not None:
            self.set_solid_mask(solid)
        if bodies is not None:
            self.set_body_labels(bodies)
        if inlet_profile is not None:
            self.set_inlet_profile(inlet_profile)
        if smagorinsky is not None:
            self.set_smagorinsky(smagorinsky)
        if trt_magic is not None:
            self.set_trt(trt_magic)
        if frames is not None:
            self.set_option("frames", frames)
        if walls is not None:
            for side, (kind, u) in zip(("south", "north"), _wall_pair(walls)):
                self.set_wall(side, kind, u)
        if inlet_schedule is not None:
            self.set_inlet_schedule(*_schedule(inlet_schedule))
        if forcing is not None:
            self.set_forcing(*forcing)
        if mrt is not None:
            self.set_mrt(*mrt)
        if sponge is not None:
            self.set_sponge(*sponge)
        if ports is not None:
            for side, (kind, v) in zip(("west", "east"), _port_pair(ports)):
                self.set_port(side, kind, v)
        if periodic_y:
            self.set_periodic_y(True)

    def _chk(self, rc):
        if rc < 0:
            raise LbmError(f"lbm_hip error {rc}: {self.L.lbm_last_error().decode()}")
        return rc

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.lbm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, key, value):
        self._chk(self.L.lbm_set_option(self.h, key.encode(), int(value)))
        if key == "frames":
            self._frames_k = int(value)

    def set_solid_mask(self, solid):
        """lbm_set_solid_mask: the global (ny, nx) mask; before initialise()."""
        m = _mask_bytes(solid, self.nx, self.ny)
        self._chk(self.L.lbm_set_solid_mask(self.h, m.ctypes.data_as(C.POINTER(C.c_ubyte)), self.nx, self.ny))

    def set_body_labels(self, labels):
        """lbm_set_body_labels: the global (ny, nx) body numbers (0 fluid, 1..255); sets the geometry too; before initialise()."""
        m = _label_bytes(labels, self.nx, self.ny)
        self._chk(self.L.lbm_set_body_labels(self.h, m.ctypes.data_as(C.POINTER(C.c_ubyte)), self.nx, self.ny))

    def body_count(self):
        """B of set_body_labels (the largest label); 0 without labels."""
        return int(self.L.lbm_body_count(self.h))

    def body_forces(self):
        """(B, 2) float64: (fx, fy) per body for t = steps_done, this strip's partial sums (lbm_get_body_forces)."""
        out = np.zeros((self.body_count(), 2), dtype=np.float64)
        self._chk(self.L.lbm_get_body_forces(self.h, _dp(out)))
        return out

    def drain_body_force_log(self, max_rows=None):
        """[(t, body, fx, fy)]: the samples step() appended beside the force log, B rows each, whole samples only."""
        if max_rows is None:
            max_rows = 4096 * max(1, self.body_count())
        rows = (BodyForceRow * max(1, max_rows))()
        n = self._chk(self.L.lbm_drain_body_force_log(self.h, rows, max_rows))
        return [(rows[k].timestep, rows[k].body, rows[k].fx, rows[k].fy) for k in range(n)]

    def set_inlet_profile(self, u):
        """lbm_set_inlet_profile: the global [ny] inlet velocities (absolute, row 0 first); before initialise()."""
        a = np.ascontiguousarray(u, dtype=np.float64)
        if a.ndim != 1:
            raise ValueError(f"inlet profile must be one-dimensional, not of shape {a.shape}")
        self._chk(self.L.lbm_set_inlet_profile(self.h, _dp(a), a.size))

    def set_smagorinsky(self, cs):
        """lbm_set_smagorinsky: the Smagorinsky constant Cs in [0, 1] (0: plain BGK); before initialise()."""
        self._chk(self.L.lbm_set_smagorinsky(self.h, float(cs)))

    def set_trt(self, magic):
        """lbm_set_trt: the TRT magic parameter (tau - 1/2)(tau_minus - 1/2) in [0, 1] (0: plain BGK); before initialise()."""
        self._chk(self.L.lbm_set_trt(self.h, float(magic)))

    def set_forcing(self, fx, fy):
        """lbm_set_forcing: the uniform driving force density (fx, fy), each of magnitude below 1 ((0, 0): none); before initialise()."""
        self._chk(self.L.lbm_set_forcing(self.h, float(fx), float(fy)))

    def set_mrt(self, bulk_rate, magic):
        """lbm_set_mrt: the bulk rate in (0, 2) and the magic parameter in (0, 1] of the MRT collision (bulk_rate 0: plain BGK); before
        initialise()."""
        self._chk(self.L.lbm_set_mrt(self.h, float(bulk_rate), float(magic)))

    def mrt(self):
        """(bulk_rate, magic) as set (lbm_get_mrt); (0.0, 0.0) without MRT."""
        sb, magic = C.c_double(), C.c_double()
        self._chk(self.L.lbm_get_mrt(self.h, C.byref(sb), C.byref(magic)))
        return sb.value, magic.value

    def set_sponge(self, width, tau_end):
        """lbm_set_sponge: the outlet sponge zone, `width` columns in 0 .. nx - 1 (0: none) over which the relaxation time rises to tau_end
        > 0.5; before initialise()."""
        self._chk(self.L.lbm_set_sponge(self.h, int(width), float(tau_end)))

    def sponge(self):
        """(width, tau_end) as set (lbm_get_sponge); (0, 0.0) without a sponge."""
        width, tau_end = C.c_int(), C.c_double()
        self._chk(self.L.lbm_get_sponge(self.h, C.byref(width), C.byref(tau_end)))
        return width.value, tau_end.value

    def sponge_rate(self, x):
        """The rate column x relaxes with, as the kernels see it (lbm_get_sponge_rate): float(T(1 / tau_x)); BGK's 1 / tau without a sponge."""
        wp = C.c_double()
        self._chk(self.L.lbm_get_sponge_rate(self.h, int(x), C.byref(wp)))
        return wp.value

    def forcing(self):
        """(fx, fy) as set (lbm_get_forcing); (0.0, 0.0) without a force."""
        fx, fy = C.c_double(), C.c_double()
        self._chk(self.L.lbm_get_forcing(self.h, C.byref(fx), C.byref(fy)))
        return fx.value, fy.value

    def set_wall(self, side, kind, velocity=0.0):
        """lbm_set_wall: side "south" (row 0) / "north" (row ny - 1); kind "no-slip" / "free-slip" / "moving" with the wall's tangential
        velocity (0 for the other kinds; "no-slip" clears a wall); before initialise()."""
        self._chk(self.L.lbm_set_wall(self.h, _wall_code(WALL_SIDES, "side", side), _wall_code(WALL_KINDS, "kind", kind), float(velocity)))

    def get_wall(self, side):
        """(kind name, velocity) of one wall (lbm_get_wall)."""
        k, u = C.c_int(), C.c_double()
        self._chk(self.L.lbm_get_wall(self.h, _wall_code(WALL_SIDES, "side", side), C.byref(k), C.byref(u)))
        return _WALL_NAMES[k.value], u.value

    def set_inlet_schedule(self, s, mode="hold"):
        """lbm_set_inlet_schedule: one scale factor of the inflow per iteration; mode "hold" (the last entry holds for ever) or "repeat"
        (periodic); an empty table clears the schedule; before initialise()."""
        a, m = _schedule((np.asarray(s, dtype=np.float64), mode))
        self._chk(self.L.lbm_set_inlet_schedule(self.h, _dp(a), a.size, m))

    def inlet_schedule_length(self):
        """Entries of the schedule as set (lbm_inlet_schedule_length); 0 without one."""
        return self.L.lbm_inlet_schedule_length(self.h)

    def inlet_scale(self, t):
        """The factor iteration t applies, in the element type (lbm_get_inlet_scale); 1.0 without a schedule."""
        v = C.c_double()
        self._chk(self.L.lbm_get_inlet_scale(self.h, int(t), C.byref(v)))
        return v.value

    def set_port(self, side, kind, value=0.0):
        """lbm_set_port: side "west" (column 0) / "east" (column nx - 1); kind "velocity" / "pressure" with the density of a pressure
        port or the velocity of the east velocity port (0 for the west velocity port, which takes inlet_velocity, the profile and the
        schedule); before initialise()."""
        self._chk(self.L.lbm_set_port(self.h, _port_code(PORT_SIDES, "side", side), _port_code(PORT_KINDS, "kind", kind), float(value)))

    def get_port(self, side):
        """(kind name, value) of one port (lbm_get_port)."""
        k, v = C.c_int(), C.c_double()
        self._chk(self.L.lbm_get_port(self.h, _port_code(PORT_SIDES, "side", side), C.byref(k), C.byref(v)))
        return _PORT_NAMES[k.value], v.value

    def set_periodic_y(self, on=True):
        """lbm_set_periodic_y: periodic top and bottom boundaries on / off; before initialise()."""
        self._chk(self.L.lbm_set_periodic_y(self.h, 1 if on is True else 0 if on is False else int(on)))

    def periodic_y(self):
        """True on a context with periodic top and bottom boundaries (lbm_get_periodic_y)."""
        return bool(self.L.lbm_get_periodic_y(self.h))

    def ports(self):
        """((west kind, value), (east kind, value)) as set; (("velocity", 0.0), ("pressure", 1.0)) on a fresh context."""
        return self.get_port("west"), self.get_port("east")

    def walls(self):
        """((south kind, velocity), (north kind, velocity)) as set; (("no-slip", 0.0), ("no-slip", 0.0)) on a fresh context."""
        return self.get_wall("south"), self.get_wall("north")

    def initialise(self):
        n = C.c_int()
        self._chk(self.L.lbm_initialise(self.h, C.byref(n)))
        self.solid_count = n.value
        self._begin_probes_kw()
        return n.value

    def _begin_probes_kw(self):
        if self._probes_kw is not None:      # the probes= keyword: begun on the initialised context
            xy, cap = self._probes_kw
            self.probes_begin(xy, self.PROBES_DEFAULT_CAPACITY if cap is None else cap)

    def step(self, nsteps=1, output_frequency=0):
        self._chk(self.L.lbm_step(self.h, nsteps, output_frequency))

    def sync(self):
        self._chk(self.L.lbm_sync(self.h))

    @property
    def steps_done(self):
        return self.L.lbm_steps_done(self.h)

    def first_unstable_step(self):
        t = C.c_int()
        self._chk(self.L.lbm_first_unstable_step(self.h, C.byref(t)))
        return t.value

    def forces(self):
        fx, fy = C.c_double(), C.c_double()
        self._chk(self.L.lbm_get_forces(self.h, C.byref(fx), C.byref(fy)))
        return fx.value, fy.value

    def drain_force_log(self, max_rows=4096):
        rows = (ForceRow * max_rows)()
        n = self._chk(self.L.lbm_drain_force_log(self.h, rows, max_rows))
        return [(rows[k].timestep, rows[k].fx, rows[k].fy) for k in range(n)]

    def macros(self):
        shape = (self.local_ny, self.nx)
        rho, ux, uy = (np.empty(shape, dtype=np.float64) for _ in range(3))
        self._chk(self.L.lbm_get_macros(self.h, _dp(rho), _dp(ux), _dp(uy)))
        return rho, ux, uy

    def max_velocity_sq(self):
        v = C.c_double()
        self._chk(self.L.lbm_max_velocity_sq(self.h, C.byref(v)))
        return v.value

    # ---- time-averaged statistics (lbm_stats_*): sampled on the device at the force-output iterations of step(n, output_frequency) ----
    def stats_begin(self, from_step=0):
        """Zeroes the six running sums and the sample count and samples every force-output iteration t >= from_step from now on."""
        self._chk(self.L.lbm_stats_begin(self.h, int(from_step)))

    def stats_end(self):
        """Stops sampling; the sums stay."""
        self._chk(self.L.lbm_stats_end(self.h))

    def stats_samples(self):
        return self._chk(self.L.lbm_stats_samples(self.h))

    def stats_sums(self):
        """(6, local_ny, nx) float64: sum of rho, ux, uy, ux*ux, uy*uy, ux*uy over the samples."""
        s = np.empty((6, self.local_ny, self.nx), dtype=np.float64)
        self._chk(self.L.lbm_get_stat_sums(self.h, _dp(s)))
        return s

    def stats_restore(self, sums, samples):
        """Uploads sums and a sample count saved earlier (a run resumed with load_state continues its averages)."""
        a = np.ascontiguousarray(sums, dtype=np.float64)
        if a.shape != (6, self.local_ny, self.nx):
            raise ValueError(f"statistics sums have shape {a.shape}, this strip needs {(6, self.local_ny, self.nx)}")
        self._chk(self.L.lbm_stats_restore(self.h, _dp(a), int(samples)))

    def stats(self):
        """{'n', 'rho', 'ux', 'uy' (means), 'uxux', 'uyuy', 'uxuy' (Reynolds stresses)} of the samples so far."""
        return _stats_from_sums(self.stats_sums(), self.stats_samples())

    # ---- coarsened flow frames (lbm_frames_*): written on the device at the force-output iterations of step(n, output_frequency) ----
    FRAMES_DEFAULT_CAPACITY = 8   # LBM_FRAMES_DEFAULT_CAPACITY

    def frames_begin(self, k, capacity=FRAMES_DEFAULT_CAPACITY):
        """From now on every force-output iteration appends one frame — rho, ux, uy and vorticity block-averaged k x k, float32 — to a
        device ring of `capacity` frames; k must divide nx, y_start and local_ny. Calling it again empties the ring."""
        self._chk(self.L.lbm_frames_begin(self.h, int(k), int(capacity)))
        self._frames_k = int(k)

    def frames_end(self):
        """Stops sampling; the undrained frames stay."""
        self._chk(self.L.lbm_frames_end(self.h))

    def frames_pending(self):
        return self._chk(self.L.lbm_frames_pending(self.h))

    def drain_frames(self, max_frames=None):
        """[(t, float32 [4, local_ny / k, nx / k])]: the oldest max_frames (default: all) undrained frames, planes rho, ux, uy, vorticity."""
        n = self.frames_pending()
        if max_frames is not None:
            n = min(n, int(max_frames))
        if n < 1:
            return []
        k = self._frames_k
        out = np.empty((n, 4, self.local_ny // k, self.nx // k), dtype=np.float32)
        ts = (C.c_int * n)()
        got = self._chk(self.L.lbm_drain_frames(self.h, ts, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return [(ts[j], out[j]) for j in range(got)]

    # ---- point probes (lbm_probes_*): sampled on the device at the force-output iterations of step(n, output_frequency) ----
    PROBES_DEFAULT_CAPACITY = 64
    PROBES_MAX = 65536            # LBM_PROBES_MAX

    def probes_begin(self, xy, capacity=PROBES_DEFAULT_CAPACITY):
        """From now on every force-output iteration appends one sample — (rho, ux, uy) in float64, interpolated bilinearly at each of the
        n points xy[j] = (x, y), GLOBAL lattice coordinates — to a device ring of `capacity` samples. Calling it again replaces the points
        and empties the ring. A strip samples the probes whose floor(y) lies in its rows and reports +0.0 for the others."""
        a = _probe_points(xy)
        self._chk(self.L.lbm_probes_begin(self.h, _dp(a), a.shape[0], int(capacity)))

    def probes_end(self):
        """Stops sampling; the undrained samples stay."""
        self._chk(self.L.lbm_probes_end(self.h))

    def probes_count(self):
        return self._chk(self.L.lbm_probes_count(self.h))

    def probes_pending(self):
        return self._chk(self.L.lbm_probes_pending(self.h))

    def drain_probes(self, max_samples=None):
        """(timesteps int32 [m], float64 [m, n, 3]): the oldest max_samples (default: all) undrained samples, (rho, ux, uy) per probe."""
        m, n = self.probes_pending(), self.probes_count()
        if max_samples is not None:
            m = min(m, int(max_samples))
        out = np.zeros((max(m, 0), n, 3), dtype=np.float64)
        ts = (C.c_int * max(m, 1))()
        got = self._chk(self.L.lbm_drain_probes(self.h, ts, _dp(out), m)) if m > 0 else 0
        return np.array(ts[:got], dtype=np.int32), out[:got]

    def populations(self, which):
        """which: 'f_current' | 'f_next' -> [(local_ny+2), (nx+2), 9] like Grid::f_current(gx,gy,i)."""
        out = np.empty((self.local_ny + 2, self.nx + 2, 9), dtype=np.float64)
        self._chk(self.L.lbm_get_populations(self.h, {"f_current": 0, "f_next": 1}[which], _dp(out)))
        return out

    def set_f_current(self, aos):
        """Write side of Grid::f_current: [(local_ny+2), (nx+2), 9]; interior cells replace the pre-collision state."""
        a = np.ascontiguousarray(aos, dtype=np.float64)
        assert a.shape == (self.local_ny + 2, self.nx + 2, 9)
        self._chk(self.L.lbm_set_f_current(self.h, _dp(a)))

    def solid(self):
        m = np.empty((self.local_ny, self.nx), dtype=np.uint8)
        self._chk(self.L.lbm_get_solid(self.h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return m

    # ---- strips ----
    def comm_unique_id(self):
        buf = (C.c_ubyte * 128)()
        self._chk(self.L.lbm_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank, nranks, id128):
        buf = (C.c_ubyte * 128).from_buffer_copy(id128)
        self._chk(self.L.lbm_comm_init(self.h, rank, nranks, buf))

    def allreduce(self, vals, op="sum"):
        a = np.ascontiguousarray(vals, dtype=np.float64)
        self._chk(self.L.lbm_comm_allreduce(self.h, _dp(a), a.size, {"sum": 0, "max": 1, "min": 2}[op]))
        return a

    HALO_ROWS = 6   # LBM_HALO_ROWS

    def halo_export(self, south=True, north=True):
        """(south_out, north_out): my bottom / top HALO_ROWS interior rows, each [HALO_ROWS, 9, nx]."""
        s = np.empty((self.HALO_ROWS, 9, self.nx), dtype=np.float64) if south else None
        n = np.empty((self.HALO_ROWS, 9, self.nx), dtype=np.float64) if north else None
        self._chk(self.L.lbm_halo_export(self.h, _dp(s), _dp(n)))
        return s, n

    def halo_import(self, south=None, north=None):
        s = np.ascontiguousarray(south, dtype=np.float64) if south is not None else None
        n = np.ascontiguousarray(north, dtype=np.float64) if north is not None else None
        self._chk(self.L.lbm_halo_import(self.h, _dp(s), _dp(n)))

    def save_state(self, path):
        self._chk(self.L.lbm_save_state(self.h, os.fspath(path).encode()))

    def load_state(self, path):
        self._chk(self.L.lbm_load_state(self.h, os.fspath(path).encode()))

    def last_step_stats(self):
        """(device ms of the last step() call, step-kernel launches it issued, iterations it advanced)."""
        ms, nl, ni = C.c_double(), C.c_int(), C.c_int()
        self._chk(self.L.lbm_last_step_stats(self.h, C.byref(ms), C.byref(nl), C.byref(ni)))
        return ms.value, nl.value, ni.value

    def last_step_dispatches(self):
        """Step kernels the launches of the last step() call ran as (a "split" plan issues a deep launch as 3 / 4 row-range kernels)."""
        return int(self.L.lbm_last_step_dispatches(self.h))

    def graph_replays(self):
        """Replays of the captured launch-group graph so far (strips with a device transport on a deep plan)."""
        return int(self.L.lbm_graph_replays(self.h))

    def last_step_kernel_ms(self):
        v = C.c_double()
        self._chk(self.L.lbm_last_step_kernel_ms(self.h, C.byref(v)))
        return v.value

    def strip_schedule(self):
        return self.L.lbm_strip_schedule(self.h).decode()

    def kernel_name(self):
        return self.L.lbm_kernel_name(self.h).decode()

    def plan(self):
        return self.L.lbm_plan(self.h).decode()

    def plan_options(self):
        """The plan as {option: value} (lbm_plan_options): with tune=0 it pins the same plan on another context."""
        return {k: int(v) for k, v in (kv.split("=") for kv in self.L.lbm_plan_options(self.h).decode().split())}


class Group:
    """n strips of one lattice driven in lockstep by this process (lbm_group_*): one Context per strip, bottom to top.
    transport: "peer" (device copies / hipMemcpyPeerAsync) or "rccl" (ncclCommInitAll; distinct devices).
    solid: optional global (ny, nx) obstacle mask, inlet_profile: optional global [ny] inlet velocities, smagorinsky: optional LES
    constant Cs, trt_magic: optional TRT magic parameter, bodies: optional global (ny, nx) body numbers (in place of solid), frames: optional frame stride k, probes / probe_capacity: optional probe points (global coordinates), walls: optional kinds of the
    bottom and top walls (as Context takes them), inlet_schedule: optional scale factors of the inflow per iteration (likewise), forcing:
    optional driving force (fx, fy), mrt: optional MRT pair (bulk_rate, magic), sponge: optional outlet sponge (width, tau_end), ports: optional pair (west, east) of the two open ends (as Context takes them), periodic_y: True joins strip
    n - 1 to strip 0 (periodic top and bottom, as Context takes it); all given to every member."""

    def __init__(self, nx, ny, bounds, devices=None, transport="peer", options=None, solid=None, inlet_profile=None, smagorinsky=None,
                 bodies=None, frames=None, trt_magic=None, probes=None, probe_capacity=None, walls=None, inlet_schedule=None, forcing=None,
                 ports=None, periodic_y=False, mrt=None, sponge=None, **kw):
        from .strips import partition_rows
        if isinstance(bounds, int):
            bounds = partition_rows(ny, bounds)
        devices = devices or [0] * len(bounds)
        self.nx, self.ny = nx, ny
        self.ctxs = [Context(nx, ny, y_start=y0, local_ny=n, device=d, options=options, solid=solid, inlet_profile=inlet_profile,
                             smagorinsky=smagorinsky, bodies=bodies, frames=frames, trt_magic=trt_magic, probes=probes,
                             probe_capacity=probe_capacity, walls=walls, inlet_schedule=inlet_schedule, forcing=forcing, ports=ports,
                             periodic_y=periodic_y, mrt=mrt, sponge=sponge, **kw)
                     for (y0, n), d in zip(bounds, devices)]
        self.L = lib()
        self._arr = (C.c_void_p * len(self.ctxs))(*[c.h for c in self.ctxs])
        self._n = len(self.ctxs)
        self._chk(self.L.lbm_group_link(self._arr, self._n, {"peer": 0, "rccl": 1}[transport]))
        self.solid_count = None

    def _chk(self, rc):
        if rc < 0:
            raise LbmError(f"lbm_hip error {rc}: {self.L.lbm_last_error().decode()}")
        return rc

    def initialise(self):
        n = C.c_int()
        self._chk(self.L.lbm_group_initialise(self._arr, self._n, C.byref(n)))
        self.solid_count = n.value
        for c in self.ctxs:
            c._begin_probes_kw()
        return n.value

    def step(self, nsteps=1, output_frequency=0):
        self._chk(self.L.lbm_group_step(self._arr, self._n, nsteps, output_frequency))

    def refresh_halos(self):
        self._chk(self.L.lbm_group_refresh_halos(self._arr, self._n))

    def sync(self):
        for c in self.ctxs:
            c.sync()

    @property
    def steps_done(self):
        return self.ctxs[0].steps_done

    # ---- the whole lattice's results: one library call each (lbm_group_get_* / lbm_group_drain_*, include/lbm_hip.h), which puts the
    # members' parts together — rows by y_start, sums in strip order, counts that must agree; g.ctxs[k] still gives a member's part ----
    def first_unstable_step(self):
        """min over the strips (the reference's MPI_Allreduce(MIN) of the stability flag, LBMGrid.h:315)."""
        t = C.c_int()
        self._chk(self.L.lbm_group_first_unstable_step(self._arr, self._n, C.byref(t)))
        return t.value

    def macros(self):
        """(rho, ux, uy) of the whole lattice: the strips' rows by y_start (LBMSolver.h:340-357)."""
        rho, ux, uy = (np.empty((self.ny, self.nx), dtype=np.float64) for _ in range(3))
        self._chk(self.L.lbm_group_get_macros(self._arr, self._n, _dp(rho), _dp(ux), _dp(uy)))
        return rho, ux, uy

    # ---- time-averaged statistics: begun and ended member by member ----
    def stats_begin(self, from_step=0):
        for c in self.ctxs:
            c.stats_begin(from_step)

    def stats_end(self):
        for c in self.ctxs:
            c.stats_end()

    def stats_samples(self):
        return self._chk(self.L.lbm_group_stats_samples(self._arr, self._n))

    def stats_sums(self):
        """(6, ny, nx): the strips' sums by y_start."""
        s = np.empty((6, self.ny, self.nx), dtype=np.float64)
        self._chk(self.L.lbm_group_get_stat_sums(self._arr, self._n, _dp(s)))
        return s

    def stats_restore(self, sums, samples):
        a = np.ascontiguousarray(sums, dtype=np.float64)
        if a.shape != (6, self.ny, self.nx):
            raise ValueError(f"statistics sums have shape {a.shape}, the lattice needs {(6, self.ny, self.nx)}")
        self._chk(self.L.lbm_group_stats_restore(self._arr, self._n, _dp(a), int(samples)))

    def stats(self):
        return _stats_from_sums(self.stats_sums(), self.stats_samples())

    # ---- coarsened flow frames: begun on every member (k must divide every strip's y_start and rows); the members sample at the same
    # iterations, and a drained frame is their rows by y_start / k ----
    def frames_begin(self, k, capacity=Context.FRAMES_DEFAULT_CAPACITY):
        for c in self.ctxs:
            c.frames_begin(k, capacity)

    def frames_end(self):
        for c in self.ctxs:
            c.frames_end()

    def frames_pending(self):
        return self._chk(self.L.lbm_group_frames_pending(self._arr, self._n))

    def drain_frames(self, max_frames=None):
        """[(t, float32 [4, ny / k, nx / k])]: the oldest max_frames (default: all) undrained frames of the whole lattice."""
        n = self.frames_pending()
        if max_frames is not None:
            n = min(n, int(max_frames))
        if n < 1:
            return []
        k = self.ctxs[0]._frames_k
        out = np.empty((n, 4, self.ny // k, self.nx // k), dtype=np.float32)
        ts = (C.c_int * n)()
        got = self._chk(self.L.lbm_group_drain_frames(self._arr, self._n, ts, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return [(ts[j], out[j]) for j in range(got)]

    # ---- point probes: every member is given the same global points and samples those of its rows (+0.0 for the others); the members
    # sample at the same iterations, and a drained sample is the SUM of theirs, like the partial force sums ----
    def probes_begin(self, xy, capacity=Context.PROBES_DEFAULT_CAPACITY):
        for c in self.ctxs:
            c.probes_begin(xy, capacity)

    def probes_end(self):
        for c in self.ctxs:
            c.probes_end()

    def probes_count(self):
        return self.ctxs[0].probes_count()

    def probes_pending(self):
        return self._chk(self.L.lbm_group_probes_pending(self._arr, self._n))

    def drain_probes(self, max_samples=None):
        """(timesteps int32 [m], float64 [m, n, 3]): the members' samples added up in strip order."""
        m, n = self.probes_pending(), self.probes_count()
        if max_samples is not None:
            m = min(m, int(max_samples))
        out = np.zeros((max(m, 0), n, 3), dtype=np.float64)
        ts = (C.c_int * max(m, 1))()
        got = self._chk(self.L.lbm_group_drain_probes(self._arr, self._n, ts, _dp(out), m)) if m > 0 else 0
        return np.array(ts[:got], dtype=np.int32), out[:got]

    def populations(self, which):
        """Ghost-inclusive [(ny+2), (nx+2), 9]: interior rows of every strip + the physical ghost rows of the end strips."""
        out = np.empty((self.ny + 2, self.nx + 2, 9), dtype=np.float64)
        self._chk(self.L.lbm_group_get_populations(self._arr, self._n, {"f_current": 0, "f_next": 1}[which], _dp(out)))
        return out

    def drain_force_log(self):
        """Rows summed over the strips (the reference's MPI_Reduce(SUM), LBMIO.h:167-168)."""
        rows = (ForceRow * 4096)()
        n = self._chk(self.L.lbm_group_drain_force_log(self._arr, self._n, rows, 4096))
        return [(rows[k].timestep, rows[k].fx, rows[k].fy) for k in range(n)]

    def forces(self):
        fx, fy = C.c_double(), C.c_double()
        self._chk(self.L.lbm_group_get_forces(self._arr, self._n, C.byref(fx), C.byref(fy)))
        return fx.value, fy.value

    # ---- per-body forces: the strips' partial sums added per (t, body) in strip order ----
    def body_count(self):
        return self.ctxs[0].body_count()

    def body_forces(self):
        """(B, 2): the strips' partial sums added in strip order."""
        out = np.zeros((self.body_count(), 2), dtype=np.float64)
        self._chk(self.L.lbm_group_get_body_forces(self._arr, self._n, _dp(out)))
        return out

    def drain_body_force_log(self):
        max_rows = 4096 * max(1, self.body_count())
        rows = (BodyForceRow * max_rows)()
        n = self._chk(self.L.lbm_group_drain_body_force_log(self._arr, self._n, rows, max_rows))
        return [(rows[k].timestep, rows[k].body, rows[k].fx, rows[k].fy) for k in range(n)]

    def max_velocity_sq(self):
        v = C.c_double()
        self._chk(self.L.lbm_group_max_velocity_sq(self._arr, self._n, C.byref(v)))
        return v.value

    def close(self):
        for c in self.ctxs:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
