"""What bench.py (the single-GPU line) and bench_launcher.py (the N > 1 launcher and its workers) share."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
W, H = 640, 480
SLAB_FORMS = ("rccl", "rccl_icp_allreduce", "direct")   # the forms of the N > 1 z-slab path (bench_launcher.py)


def host_cores():
    """the CPU cores this process can really use: its affinity mask, cut down to the container's CPU quota (cgroup v2
    cpu.max / v1 cfs quota) -- 256 OpenMP threads on a 16-core quota run 30 times slower than 16"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(p)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / p
        except (OSError, ValueError):
            pass
    if quota is not None:
        n = max(1, min(n, int(quota + 0.5)))
    return n


def synth_frames(hsk, first, count):
    """frames first .. first + count - 1 of the scripted stream, hsk.synth_depth(hsk.synth_pose(k)) bit for bit, in a time
    that hardly grows with count: a frame is a function of its float32 pose alone and the scripted poses repeat (300
    distinct ones in the first 300 frames, 825 in the first 20000), so each distinct pose is rendered once, on the host
    cores this process may use (hsk_synth_render runs outside the GIL).
    -> (poses, distinct frames [U, H, W] uint16, index [count] of every frame's distinct one)"""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    poses = [hsk.synth_pose(k) for k in range(first, first + count)]
    slot, distinct = {}, []
    index = np.empty(count, np.int64)
    for k, p in enumerate(poses):
        index[k] = slot.setdefault(p.tobytes(), len(distinct))
        if index[k] == len(distinct):
            distinct.append(p)
    with ThreadPoolExecutor(max_workers=host_cores()) as ex:
        rendered = np.stack(list(ex.map(hsk.synth_depth, distinct)))
    return poses, rendered, index


def make_frames(hsk, first, count):
    """(poses, frames) of the scripted stream; repeated frames are views of one read-only array"""
    poses, distinct, index = synth_frames(hsk, first, count)
    distinct.flags.writeable = False
    return poses, [distinct[j] for j in index]


def check_build(args):
    """The measured library must be the default build of THIS tree: "+exp" marks other compiler flags (timing experiments,
    some of which give wrong results by construction), a different hash a stale .so.  tests/conftest.py refuses both too."""
    from housescan_amd import _lib
    from housescan_amd.csrc import build_id as tree_id
    have, want = _lib.load().hsk_build_id().decode(), tree_id.build_id()
    if have != want and not args.allow_exp:
        raise SystemExit("bench.py: housescan_amd/libhskinfu.so is build %s, the tree is %s -- rebuild with "
                         "`python -c 'import __graft_entry__ as g; g.build()'` (or pass --allow-exp for a timing experiment)" % (have, want))
    return have


def emit(out, have=None, want=None):
    """the JSON line is the LAST thing on stdout: RCCL's version banner sits in the C library's buffer until then"""
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    print(json.dumps(out))
    sys.stdout.flush()
