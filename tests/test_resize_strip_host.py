"""k_resize_strip's geometry without a GPU: tests/_probe/resize_strip_host.cpp runs the library's own build_geometry and strip choice
(orbx_geometry.hip over tests/_probe/hip_stub) on a few thousand random image geometries under AddressSanitizer + UndefinedBehaviorSanitizer
and replays the kernel's lane maps (orb_slam_amd/csrc/k_resize_strip.h) on the CPU: the staged range stays inside the source rows' promised
bytes, every tap's three-dword window inside the LDS tile, the tile inside the budget, strips and lanes partition the level, and a level
takes the strip form exactly when the windowed form applies, the source is 4-byte aligned and twelve rows and more fit the budget."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resize_strip_geometry(tmp_path):
    exe = str(tmp_path / "resize_strip_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-attributes", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__host__=", "-D__device__=", "-o", exe,
           "-I" + os.path.join(ROOT, "tests", "_probe", "hip_stub"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "orb_slam_amd", "csrc"), os.path.join(ROOT, "tests", "_probe", "resize_strip_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "resize strip host ok" in r.stdout
    m = re.search(r"built (\d+) levels (\d+) strip_levels (\d+) strips (\d+) rowpar_levels (\d+) tail_strips (\d+) failures 0", r.stdout)
    assert m and int(m.group(1)) >= 1500 and int(m.group(3)) >= 1000, r.stdout      # the sample really holds eligible levels, of both lane maps
