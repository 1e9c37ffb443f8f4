"""Host-side mirror of the reference's simulator loop for a batch of worlds.

``WorldBatch.step(dt, nsteps)`` plays the role of calling
``TimeSteppingSimulator::step(dt)`` (include/Moby/TimeSteppingSimulator.h:36)
``nsteps`` times on every world; ``regress_rows`` formats the state the way
``programs/regress.cpp:82-93`` prints it (t, then x y z qx qy qz qw per body).
"""
import ctypes

import numpy as np

from . import _lib
from . import scene as S


REPORT_PAIR = 8      # MH_REPORT_PAIR: doubles per (world, step, pair slot) row of the contact report (include/moby_hip.h, "Contact report")


def report_npt(scene, statics=None):
    """pair slots of a scene: triangular over ntot = nb + has_ground + n bodies"""
    ntot = scene.nb + (1 if scene.has_ground else 0) + (statics.n if statics is not None else 0)
    return ntot * (ntot - 1) // 2


def body_impulses(report, nb, ntot):
    """Net linear contact impulse per enabled body from a contact report (..., npt, 8) -> (..., nb, 3): row [2..4] of pair slot (i, j) is the impulse on
    body i; body j, if it is a body (j < nb), received the negative.  Array operators only: numpy arrays and torch tensors alike."""
    shape = tuple(report.shape[:-2]) + (nb, 3)
    out = report.new_zeros(shape) if hasattr(report, "new_zeros") else np.zeros(shape, dtype=report.dtype)   # (the one line that asks which of the two)
    p = 0
    for i in range(ntot):
        for j in range(i + 1, ntot):
            if i < nb:
                out[..., i, :] = out[..., i, :] + report[..., p, 2:5]
            if j < nb:
                out[..., j, :] = out[..., j, :] - report[..., p, 2:5]
            p += 1
    return out


class WorldBatch:
    """B worlds of one scene; numpy host arrays in/out (copies through the library)."""

    def __init__(self, scene, state, aux=None, seed=1, forces=None, statics=None, params=None):
        self.scene = scene
        self.state = np.ascontiguousarray(state, dtype=np.float64)
        self.B = self.state.shape[0]
        assert self.state.shape[1] == scene.nb * S.MH_BODY_STATE
        self.aux = S.new_aux(self.B, seed) if aux is None else aux
        self.forces = forces       # S.mh_world_forces (S.make_forces) or None: the scene's recurrent forces
        self.statics = statics     # S.mh_world_statics (S.make_statics, io.load_xml_statics) or None: static bodies beside the scene's ground
        self.params = None if params is None else S.params_array(params, self.B)   # S.PARAMS_DTYPE records (S.make_params), one per world, or None

    def step(self, dt, nsteps=1, want_traj=False, wrench=None, want_report=False):
        """wrench: (B, nb, 6) or (rows >= nsteps, B, nb, 6) host array (fx fy fz tx ty tz per world and body), or None.
        want_report: returns (trajectory or None, report) with the contact report (B, nsteps, npt, 8) of include/moby_hip.h, "Contact report"."""
        if wrench is not None:
            return self._step_wrench(dt, nsteps, want_traj, wrench, want_report)
        # the host convenience with every optional argument: NULL for what the batch has not (a NULL report keeps it off the report build)
        traj = np.zeros((self.B, nsteps, self.scene.nb, 7)) if want_traj else None
        report = np.zeros((self.B, nsteps, report_npt(self.scene, self.statics), REPORT_PAIR)) if want_report else None
        _lib.check(_lib.load().mh_world_step_batch_report(ctypes.addressof(self.scene), None if self.forces is None else ctypes.addressof(self.forces),
                                                          None if self.statics is None else ctypes.addressof(self.statics),
                                                          None if self.params is None else self.params.ctypes.data,
                                                          self.B, float(dt), int(nsteps), self.state.ctypes.data, self.aux.ctypes.data,
                                                          None if traj is None else traj.ctypes.data, None if report is None else report.ctypes.data))
        return (traj, report) if want_report else traj

    def _step_wrench(self, dt, nsteps, want_traj, wrench, want_report):
        """a wrench is a DEVICE array: the same round trip through a device batch (created for the report if one is wanted)"""
        import torch
        dev = WorldBatchDevice(self.scene, self.state, aux=self.aux, statics=self.statics, params=self.params, report=want_report)
        try:
            if self.forces is not None:
                dev.set_forces(self.forces)
            traj = torch.zeros((self.B, nsteps, self.scene.nb, 7), dtype=torch.float64, device="cuda") if want_traj else None
            report = torch.zeros((self.B, nsteps, dev.npt, REPORT_PAIR), dtype=torch.float64, device="cuda") if want_report else None
            w = torch.as_tensor(np.ascontiguousarray(wrench, dtype=np.float64), device="cuda")
            dev.step(dt, nsteps, traj_ptr=None if traj is None else traj.data_ptr(), wrench=w, report=report)
            self.state[...], aux = dev.download()
            self.aux[...] = aux
        finally:
            dev.close()
        traj = None if traj is None else traj.cpu().numpy()
        return (traj, report.cpu().numpy()) if want_report else traj

    def regress_rows(self):
        """(B, 1 + 7*nb): current_time followed by the Euler coordinates of every body."""
        q = self.state.reshape(self.B, self.scene.nb, S.MH_BODY_STATE)[:, :, :7].reshape(self.B, -1)
        return np.concatenate([self.aux["time"][:, None], q], axis=1)


class WorldBatchDevice:
    """Same, with state/aux resident in HBM behind an ``mh_world_batch`` handle;
    ``step`` is asynchronous on the given (torch) stream."""

    def __init__(self, scene, state, seed=1, aux=None, statics=None, params=None, report=False):
        """report: the batch is created for the contact report (mh_world_batch_create_report): step / step_ids take report="""
        lib = _lib.load()
        self.scene = scene
        self.B = state.shape[0]
        self.handle = ctypes.c_void_p()
        self.npt = report_npt(scene, statics)
        p = None if params is None else S.params_array(params, self.B)
        create = lib.mh_world_batch_create_report if report else lib.mh_world_batch_create_params      # (NULL for what the batch has not)
        _lib.check(create(ctypes.addressof(scene), None if statics is None else ctypes.addressof(statics), None if p is None else p.ctypes.data, self.B,
                          ctypes.byref(self.handle)))
        self.device = lib.mh_world_batch_device(self.handle)      # the HIP device the batch lives on: device tensors handed to it must be that device's
        st = np.ascontiguousarray(state, dtype=np.float64)
        aux = S.new_aux(self.B, seed) if aux is None else np.ascontiguousarray(aux)      # aux given: resume from a checkpoint
        _lib.check(lib.mh_world_batch_upload(self.handle, st.ctypes.data, aux.ctypes.data))

    def set_forces(self, forces):
        """The scene's recurrent forces (S.mh_world_forces from S.make_forces / io.load_xml_forces; None clears them): every later step honours them."""
        _lib.check(_lib.load().mh_world_batch_set_forces(self.handle, None if forces is None else ctypes.addressof(forces)))

    def set_params(self, params, first=0):
        """Replaces the records of worlds first .. first + len(params) (a host array of S.PARAMS_DTYPE; validated by the library).  The batch must have been
        created with params=; not while a launch is in flight."""
        p = S.params_array(params)
        _lib.check(_lib.load().mh_world_batch_set_params(self.handle, p.ctypes.data, int(first), int(p.shape[0])))

    def set_params_dev(self, params, first=0, count=None, stream=None):
        """The same from DEVICE memory, an asynchronous copy on `stream`, NOT validated (include/moby_hip.h): a contiguous float64 tensor on the batch's
        device shaped (count, S.PARAMS_DOUBLES), or a raw device pointer with `count` given."""
        if hasattr(params, "data_ptr"):
            if not (params.is_cuda and params.is_contiguous() and str(params.dtype) == "torch.float64"):
                raise ValueError("params: a contiguous float64 tensor on the device is needed")
            shape = tuple(params.shape)
            if len(shape) != 2 or shape[1] != S.PARAMS_DOUBLES or (count is not None and int(count) != shape[0]):
                raise ValueError("params: shape %s, expected (%s, %d)" % (shape, "count" if count is None else int(count), S.PARAMS_DOUBLES))
            ptr, count = ctypes.c_void_p(params.data_ptr()), shape[0]
        else:
            if count is None:
                raise ValueError("params: a raw device pointer needs count")
            ptr = ctypes.c_void_p(int(params))
        _lib.check(_lib.load().mh_world_batch_set_params_dev(self.handle, stream, ptr, int(first), int(count)))

    def _on_device(self, t, name):
        """a contiguous float64 tensor on the batch's own device, or ValueError"""
        if not (hasattr(t, "data_ptr") and t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.float64"):
            raise ValueError("%s: a contiguous float64 tensor on the device is needed" % name)
        if t.device.index != self.device:
            raise ValueError("%s: the tensor is on device %s, the batch on device %d" % (name, t.device.index, self.device))

    def _wrench_args(self, wrench, rows):
        """(device pointer, rows) of a wrench schedule: a float64 torch tensor on the batch's device shaped (B, nb, 6) or (rows, B, nb, 6), or a raw
        device pointer with `rows` given (rows x B x nb x 6 doubles)."""
        if hasattr(wrench, "data_ptr"):
            nb = self.scene.nb
            self._on_device(wrench, "wrench")
            shape = tuple(wrench.shape)
            if shape == (self.B, nb, 6):
                shape = (1,) + shape
            if shape[1:] != (self.B, nb, 6) or (rows is not None and int(rows) != shape[0]):
                raise ValueError("wrench: shape %s, expected ([rows,] %d, %d, 6)" % (tuple(wrench.shape), self.B, nb))
            return ctypes.c_void_p(wrench.data_ptr()), shape[0]
        return ctypes.c_void_p(int(wrench)), 1 if rows is None else int(rows)

    def _report_ptr(self, report, nsteps):
        """device pointer of a report tensor: contiguous float64 on the batch's device, shaped (B, nsteps, npt, 8) -- B the worlds of the batch"""
        self._on_device(report, "report")
        want = (self.B, int(nsteps), self.npt, REPORT_PAIR)
        if tuple(report.shape) != want:
            raise ValueError("report: shape %s, expected %s" % (tuple(report.shape), want))
        return ctypes.c_void_p(report.data_ptr())

    def _launch(self, dt, nsteps, stream, traj_ptr, ids_ptr, count, wrench, rows, report):
        """the stepping entry with every optional argument (mh_world_batch_step_report): NULL for what the launch has not"""
        wptr, rows = (None, 1) if wrench is None else self._wrench_args(wrench, rows)
        _lib.check(_lib.load().mh_world_batch_step_report(self.handle, stream, float(dt), int(nsteps), traj_ptr, ids_ptr, int(count), wptr, rows,
                                                          None if report is None else self._report_ptr(report, nsteps)))

    def step(self, dt, nsteps=1, stream=None, traj_ptr=None, wrench=None, rows=None, report=None):
        """wrench: per-world body wrenches for this launch (see _wrench_args; rows == 1 holds for the launch, rows >= nsteps is one row per step).
        report: the contact report of this launch (see _report_ptr; a batch created with report=True)."""
        self._launch(dt, nsteps, stream, traj_ptr, None, 0, wrench, rows, report)

    def step_ids(self, dt, nsteps, ids_dev_ptr, count, stream=None, wrench=None, rows=None, report=None):
        """nsteps of the worlds listed in a DEVICE int32 array (e.g. a torch tensor's data_ptr()) on `stream` (mh_world_batch_step_ids); with a
        wrench, each listed world reads the schedule at its own index in the batch; with a report (the whole batch's shape), only the listed worlds'
        rows are written, each at its own index in the batch."""
        ids_ptr = ctypes.c_void_p(int(ids_dev_ptr))
        if wrench is None and report is None:      # (its own entry: it refuses a null id list, and words its count / step refusals its own way)
            _lib.check(_lib.load().mh_world_batch_step_ids(self.handle, stream, float(dt), int(nsteps), ids_ptr, int(count)))
            return
        self._launch(dt, nsteps, stream, None, ids_ptr, count, wrench, rows, report)

    def occupancy(self):
        """resident workgroups per CU of the kernel this batch launches now (runtime query; the forced kernel once forces are stored)"""
        n = _lib.load().mh_world_batch_occupancy(self.handle)
        if n < 0:
            _lib.check(n)
        return n

    def download(self):
        st = np.zeros((self.B, self.scene.nb * S.MH_BODY_STATE))
        aux = np.zeros(self.B, dtype=S.AUX_DTYPE)
        _lib.check(_lib.load().mh_world_batch_download(self.handle, st.ctypes.data, aux.ctypes.data))
        return st, aux

    def close(self):
        if self.handle:
            _lib.load().mh_world_batch_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass



def save_checkpoint(path, scene, state, aux):
    """Everything a resumed run needs: the scene record, the body states and the per-world solver state
    (``mh_world_aux``: rand() stream, _zlast / _z / _v with their sizes, current_time, status, counters).  The reference's
    XML pickle (programs/driver.cpp:224-232) keeps none of the solver state, so its resumed runs diverge in pivot sequence."""
    np.savez(path, scene=np.frombuffer(bytes(scene), dtype=np.uint8), state=np.ascontiguousarray(state, dtype=np.float64),
             aux=np.frombuffer(np.ascontiguousarray(aux).tobytes(), dtype=np.uint8), nworlds=np.int64(len(aux)))


def load_checkpoint(path):
    """Returns (scene, state, aux) as ``save_checkpoint`` stored them."""
    z = np.load(path)
    scene = S.mh_scene.from_buffer_copy(z["scene"].tobytes())
    aux = np.frombuffer(z["aux"].tobytes(), dtype=S.AUX_DTYPE).copy()
    assert len(aux) == int(z["nworlds"])
    return scene, z["state"].copy(), aux
