"""oracle.build() when several processes need the library at once.

The spawned ranks of tests/test_halo_gloo.py all import the oracle at the same moment.  If the library is missing or
older than its source, each of them used to run make in the same directory: one linked while another loaded
("file too short"), or one rewrote an object file under the other's link (a library without its f32 half).  build()
now serialises on a lock and the Makefile moves the finished library into place.  The race is run here in a private
copy of oracle/, so the library the rest of the suite uses is left alone.
"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LOAD = """
import sys
sys.path.insert(0, sys.argv[1])
from oracle import oracle as O
import numpy as np
L = O.lib()
for suf, dt in (("f64", np.float64), ("f32", np.float32)):
    assert hasattr(L, "ns3d_ref_update_tau_" + suf)
    a = np.asfortranarray(np.arange(-3, 5, dtype=dt).reshape(2, 2, 2))
    assert O.max_abs(a) == 4.0
print("loaded")
"""


def test_concurrent_first_builds_all_load_a_whole_library(tmp_path):
    dst = tmp_path / "oracle"
    dst.mkdir()
    for f in ("__init__.py", "oracle.py", "Makefile", "ns3d_oracle.c"):
        shutil.copy(os.path.join(ROOT, "oracle", f), dst / f)
    env = {k: v for k, v in os.environ.items() if k != "NS3D_ORACLE_LIB"}
    procs = [subprocess.Popen([sys.executable, "-c", _LOAD, str(tmp_path)], env=env, cwd=str(tmp_path),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for _ in range(6)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0 and out.strip().endswith("loaded"), out
    left = sorted(os.listdir(dst))
    assert "libns3d_oracle.so" in left and not [f for f in left if f.startswith("tmp.")], left
