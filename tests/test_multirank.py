"""N>1 path: row strips, one process per strip, halo exchange every step. World size 2 (and 3) over gloo on the
CPU with the oracle as the per-strip engine; on the GPU box the same worker drives two HIP contexts (host-staged
halos over gloo, both ranks on the one GPU) and, where RCCL accepts two ranks on one device, the RCCL path."""
import importlib
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.helpers import PKG, ROOT

WORKER = os.path.join(ROOT, "tests", "_mr_worker.py")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(backend, world, nx, ny, steps, of, timeout=300):
    out = os.path.join(tempfile.mkdtemp(prefix="lbm_mr_"), "out.npz")
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, WORKER, backend, str(nx), str(ny), str(steps), str(of), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs, codes = [], []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
        codes.append(p.returncode)
    return codes, logs, out


def single_domain_oracle(nx, ny, steps, of):
    from oracle.oracle import Oracle, make_params
    o = Oracle(make_params(nx, ny, tau=0.6, inlet_velocity=0.06, cylinder_radius=0.12))
    forces = []
    assert o.run(steps, of, forces) == -1
    return o, forces


def test_partition_rows():
    lbm = importlib.import_module(PKG)
    assert lbm.partition_rows(1024, 8) == [(128 * r, 128) for r in range(8)]
    assert lbm.partition_rows(10, 3) == [(0, 4), (4, 3), (7, 3)]
    parts = lbm.partition_rows(1000, 7)
    assert sum(n for _, n in parts) == 1000 and all(parts[k][0] + parts[k][1] == parts[k + 1][0] for k in range(6))
    with pytest.raises(ValueError):
        lbm.partition_rows(3, 4)


@pytest.mark.parametrize("world", [2, 3])
def test_strips_over_gloo_cpu(world):
    """world_size-2/3 gloo run of the strip protocol (only populations {2,5,6}/{4,7,8} travel) == 1 domain, bitwise."""
    nx, ny, steps, of = 96, 50, 60, 20
    codes, logs, out = launch("oracle", world, nx, ny, steps, of)
    assert codes == [0] * world, "\n".join(logs)
    z = np.load(out)
    o, forces = single_domain_oracle(nx, ny, steps, of)
    assert np.array_equal(z["rho"], o.rho) and np.array_equal(z["ux"], o.ux) and np.array_equal(z["uy"], o.uy)
    ref = np.array([[r[1], r[2]] for r in forces])
    assert np.allclose(z["forces"], ref, rtol=0, atol=1e-14)


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["hip-host", "hip-host-pair", "hip-rccl"])
def test_two_ranks_on_the_gpu(backend):
    """Two processes, two strips, both on device 0. hip-host: halos staged through the host over gloo. hip-rccl:
    the production RCCL send/recv path; RCCL may refuse two ranks on one device (then the test is skipped — the
    multi-GPU run itself belongs to the driver's 8-GPU node)."""
    nx, ny, steps, of = 512, 128, 80, 20
    codes, logs, out = launch(backend, 2, nx, ny, steps, of)
    if backend == "hip-rccl" and 77 in codes:
        pytest.skip("RCCL refused two ranks on one device: " + " | ".join(l.strip().splitlines()[-1] for l in logs if l.strip()))
    assert codes == [0, 0], "\n".join(logs)
    z = np.load(out)
    o, forces = single_domain_oracle(nx, ny, steps, of)
    from tests.helpers import macro_errors
    er, eu = macro_errors(z["rho"], z["ux"], z["uy"], o.rho, o.ux, o.uy)
    assert er < 1e-10 and eu < 1e-10, (er, eu)
    ref = np.array([[r[1], r[2]] for r in forces])
    assert np.allclose(z["forces"], ref, rtol=0, atol=1e-10 * np.abs(ref).max())
