"""float64 statement of ops.mask_aggregate (csrc/mp_mask.h) on numpy arrays that hold the stored values, and
the plan of mp_mask.h through a small host library (tests/csrc/mask_plan_check.cc)."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "euler_amd", "csrc")


def unpack(mask, m):
    """[rows, words] 64-bit words -> bool [rows, m]: bit c % 64 of word c // 64, the bits >= m dropped"""
    words = np.ascontiguousarray(mask).view(np.uint64)
    bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(words.shape[0], -1)[:, :m].astype(bool)


def pack(bits):
    """bool [rows, m] -> int64 [rows, (m + 63) // 64]"""
    rows, m = bits.shape
    full = np.zeros((rows, (m + 63) // 64 * 64), np.uint64)
    full[:, :m] = bits
    return (full.reshape(rows, -1, 64) << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64).view(np.int64)


def mask_aggregate_ref(op, mask, x, root, batch, n, m, dtype=np.float64):
    """-> (out [batch * n, d], deg [batch * n], sum of |terms| [batch * n, d]); S is summed in float64, the
    epilogue (root add, the one division) runs in `dtype`"""
    bits = unpack(mask, m).reshape(batch, n, m).astype(np.float64)
    xs = np.asarray(x, np.float64)[:batch * m].reshape(batch, m, -1)
    s = np.einsum("bnm,bmd->bnd", bits, xs).reshape(batch * n, -1).astype(dtype)
    mag = np.einsum("bnm,bmd->bnd", bits, np.abs(xs)).reshape(batch * n, -1)
    deg = bits.sum(2).reshape(-1, 1).astype(dtype)
    r = None if root is None else np.asarray(root, np.float64).astype(dtype)
    lo = np.maximum(deg, dtype(1e-7))
    out = {"add": lambda: s, "mean": lambda: s / lo, "gcn": lambda: r + s / lo,
           "gcn_renorm": lambda: (r + s) / (dtype(1) + deg)}[op]()
    return out, deg.reshape(-1), mag + (0 if r is None else np.abs(r))


@functools.lru_cache(None)
def plan_lib():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out_dir = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so, src = os.path.join(out_dir, "libmask_plan_check.so"), os.path.join(HERE, "csrc", "mask_plan_check.cc")
    deps = [src] + [os.path.join(CSRC, h) for h in ("mp_mask.h", "mp_dense.h", "mp_pool.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, src, "-o", so])
    lib = C.CDLL(so)
    lib.mask_plan.argtypes = [C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int32)]
    lib.mask_tile.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    return lib


def plan(m, d, f32):
    """-> (nt, column tiles, candidate block, stride, LDS bytes) of MaskMakePlan"""
    out = (C.c_int32 * 5)()
    plan_lib().mask_plan(m, d, int(f32), out)
    return tuple(out)
