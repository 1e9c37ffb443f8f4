"""The box reference's ctypes face (tests/native/artic_box_ref.cpp), shared by the CPU and the GPU tests of box primitives on links."""
import ctypes

import numpy as np

from moby_amd import artic as A
from tests import native_build



class BoxRef:
    """ctypes face of tests/native/artic_box_ref.cpp"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.artic_box_ref_step.restype = None

    def step(self, model, q, qd, aux, dt, nsteps, pose=None, drive=None):
        keep = None
        d = None
        if drive is not None:
            drive.check(q.shape[0], model.nj)
            d = A.mh_artic_drive(terms=drive.terms, rows=drive.rows)
            keep = {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in drive.arrays.items() if a is not None}
            for k, a in keep.items():
                setattr(d, k, a.ctypes.data)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self.lib.artic_box_ref_step(ctypes.byref(model), int(q.shape[0]), ctypes.c_double(dt), int(nsteps), P(q), P(qd), P(aux),
                                    None if pose is None else P(pose), None if d is None else ctypes.byref(d))
        del keep


def build_box_ref():
    return BoxRef(native_build.build(("artic_box_ref.cpp", "artic_drive_ref.cpp", "artic_pose_ref.cpp"), "artic_box_ref"))
