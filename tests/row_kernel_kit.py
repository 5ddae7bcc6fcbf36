"""What the case modules of the stand-alone row kernels share (tests/com_task_cases.py, manipulability_cases.py,
rolling_cases.py): the error measure against a 60-digit reference, the configurations, the recorder of measured ratios and
the emulator behind the BatchSolver methods of the three kernels."""
import ctypes
import json
import os

import mpmath as mp
import numpy as np

from oracle import exact_kinematics as ek
from pink_amd._lib import PinkHipError

EPS = 2.0 ** -52


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _split(ref):
    """An exact (mpf) result as doubles (hi, lo): hi the nearest double of every entry, lo what it leaves."""
    fl = ek.flat(ref)
    hi = np.array([float(x) for x in fl])
    with mp.workdps(ek.DPS):
        lo = np.array([float(x - mp.mpf(h)) for x, h in zip(fl, hi)])
    return hi, lo


def ratio(dev, ref, S):
    """Error in units of u = S + eps max|reference| (tests/test_kinematics_exact.py)."""
    hi, lo = ref
    u = S + EPS * np.abs(hi).max()
    return float(np.abs((np.asarray(dev, dtype=np.float64).ravel() - hi) - lo).max() / u)


def random_configurations(model, B, rng):
    """Revolute angles over a few turns, prismatic coordinates in +-0.5, free-flyer quaternions with w < 0."""
    q = np.zeros((B, model.nq))
    for j in model.joints:
        if j.kind == "free_flyer":
            q[:, j.idx_q:j.idx_q + 3] = rng.normal(size=(B, 3))
            qu = rng.normal(size=(B, 4))
            qu[:, 3] = -np.abs(qu[:, 3]) - 0.1
            q[:, j.idx_q + 3:j.idx_q + 7] = qu / np.linalg.norm(qu, axis=1, keepdims=True)
        elif j.kind == "prismatic":
            q[:, j.idx_q] = rng.uniform(-0.5, 0.5, size=B)
        else:
            q[:, j.idx_q] = rng.uniform(-6.0, 6.0, size=B)
    return q


class RatioRecorder:
    """The worst ratios a session measures, as ``noted[who]["<case>_<key>"]``.  ``write`` merges them into the JSON file the
    environment variable ``env`` names, one block per ``who`` ("host" / "emu" / "gpu" / ...: the host tests and the device
    tests of one session, and a later GPU session, add theirs); ``profile``: where the repository keeps that file.
    ``merge``: a block keeps the entries this session did not measure.  ``extra``: () -> further top-level entries."""

    def __init__(self, env, profile, keys, merge=False, extra=None):
        self.env, self.profile, self.keys, self.merge, self.extra, self.noted = env, profile, keys, merge, extra, {}

    def note(self, who, name, *ratios):
        d = self.noted.setdefault(who, {})
        for key, v in zip(self.keys, ratios):
            if v is not None:
                d[f"{name}_{key}"] = max(d.get(f"{name}_{key}", 0.0), float(v))

    def write(self):
        path = os.environ.get(self.env)
        if not path or not self.noted:
            return
        have = {}
        if os.path.exists(path):
            with open(path) as f:
                have = json.load(f)
        for who, d in self.noted.items():
            block = {n: float("%.3g" % v) for n, v in sorted(d.items())}
            have[who] = {**have.get(who, {}), **block} if self.merge else block
        if self.extra:
            have.update(self.extra())
        with open(path, "w") as f:
            json.dump(have, f, indent=1, sort_keys=True)
            f.write("\n")


# ---- the emulator behind BatchSolver's row-kernel methods (EmuSolver lives in conftest.py: its methods are added here) ----
def _emu(api, **argtypes):
    """(lib, check) of the emulator behind ``api`` with the argument types of its entry points set."""
    lib = api.lib
    for name, types in argtypes.items():
        getattr(lib, name).argtypes = types
    lib.pinkhip_emu_last_error.restype = ctypes.c_char_p

    def check(rc):
        if rc != 0:
            raise PinkHipError(rc, lib.pinkhip_emu_last_error().decode())

    return lib, check


VP, LL, CI = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int


def with_com(api):
    """The three centre-of-mass methods (com_create / com_destroy / com_task)."""
    if hasattr(api, "com_task"):
        return api
    lib, check = _emu(api, pinkhip_emu_com_create=[VP, CI, VP, VP, ctypes.POINTER(VP)], pinkhip_emu_com_destroy=[VP],
                      pinkhip_emu_com_task=[VP, VP, LL, VP, VP, CI, VP, LL, VP, LL, CI, VP])

    def com_create(model, mass, com):
        mass = np.ascontiguousarray(mass, dtype=np.float64)
        com = np.ascontiguousarray(com, dtype=np.float64)
        if mass.ndim != 1 or com.shape != (mass.shape[0], 3):
            raise ValueError(f"mass [nj] and com [nj, 3] expected, got {mass.shape} and {com.shape}")
        c = VP()
        check(lib.pinkhip_emu_com_create(model, mass.shape[0], mass.ctypes.data, com.ctypes.data, ctypes.byref(c)))
        return c.value

    def com_task(model, com, B, q, target, target_batched, e, sE, J, sJ, row0, com_out=None):
        check(lib.pinkhip_emu_com_task(model, com, B, q, target, int(bool(target_batched)), e, sE, J, sJ, int(row0), com_out))

    api.com_create, api.com_task = com_create, com_task
    api.com_destroy = lambda c: lib.pinkhip_emu_com_destroy(VP(c))
    return api


def with_manipulability(api):
    """``manipulability_task`` (pinkhip_manipulability_task_device's twin on host memory)."""
    if hasattr(api, "manipulability_task"):
        return api
    lib, check = _emu(api, pinkhip_emu_manipulability_task=[VP, LL, VP, CI, CI, CI, ctypes.c_double, VP, LL, VP, LL, CI, VP])

    def manipulability_task(model, B, q, frame, reference_frame, row_mask, rate, e, sE, J, sJ, row0, m_out=None):
        check(lib.pinkhip_emu_manipulability_task(model, B, q, int(frame), int(reference_frame), int(row_mask), float(rate), e, sE, J, sJ,
                                                  int(row0), m_out))

    api.manipulability_task = manipulability_task
    return api


def with_rolling(api):
    """``rolling_tasks`` (pinkhip_rolling_tasks_device's twin on host memory)."""
    if hasattr(api, "rolling_tasks"):
        return api
    lib, check = _emu(api, pinkhip_emu_rolling_tasks=[VP, LL, VP, CI, VP, VP, VP, VP, LL, VP, LL, CI, VP])

    def rolling_tasks(model, B, q, slots, kinds, radii, e, sE, J, sJ, row0, height_out=None):
        n = len(slots)
        s, k, r = (None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in ((slots, np.int32), (kinds, np.int32), (radii, np.float64)))
        check(lib.pinkhip_emu_rolling_tasks(model, B, q, n, *(None if a is None else a.ctypes.data for a in (s, k, r)), e, sE, J, sJ, int(row0),
                                            height_out))

    api.rolling_tasks = rolling_tasks
    return api


def with_row_kernels(api):
    """All of the above (a GPU solver has the methods already and comes back as it is)."""
    return with_rolling(with_manipulability(with_com(api)))
