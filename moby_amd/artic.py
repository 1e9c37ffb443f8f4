"""Host-side mirror of the articulated-body stepper (include/moby_hip_artic.h).

``ArticBatch(model, q, qd)`` plays the role of B simulators that each hold one fixed-base ``RCArticulatedBody``
(``step``, driven by joint forces and PD servos through a ``Drive``), and of ``RCArticulatedBodyd::calc_fwd_dyn`` / ``get_generalized_inertia`` on their states (``fwd_dyn``);
``load_sdf`` reads example/ur10/model.sdf through the C++ loader of libmoby_hip_io.so; ``model_from_links`` builds a
model from global link poses the way that loader does (synthetic chains for the tests).
"""
import ctypes
import os

import numpy as np

from . import _lib
from . import io as mio
from . import scene as S

MH_ARTIC_MAX_JOINTS = 16
MH_JOINT_REVOLUTE, MH_JOINT_PRISMATIC = 0, 1
MH_ARTIC_MAX_SPHERES = 4
MH_ARTIC_MAX_BOXES = 8
MH_ARTIC_MAX_PAIRS = 6
MH_ARTIC_PAIR_SPHERES, MH_ARTIC_PAIR_BOX_SPHERE = 0, 1      # mh_artic_model.pair_kind
_NJ = MH_ARTIC_MAX_JOINTS
_NS = MH_ARTIC_MAX_SPHERES
_NB = MH_ARTIC_MAX_BOXES
_NP = MH_ARTIC_MAX_PAIRS


class mh_artic_model(ctypes.Structure):
    _fields_ = [("nj", ctypes.c_int), ("parent", ctypes.c_int * _NJ), ("jtype", ctypes.c_int * _NJ),
                ("Rrel", (ctypes.c_double * 9) * _NJ), ("trel", (ctypes.c_double * 3) * _NJ), ("axis", (ctypes.c_double * 3) * _NJ),
                ("com", (ctypes.c_double * 3) * _NJ), ("inertia", (ctypes.c_double * 9) * _NJ), ("mass", ctypes.c_double * _NJ),
                ("lolimit", ctypes.c_double * _NJ), ("hilimit", ctypes.c_double * _NJ), ("limit_restitution", ctypes.c_double * _NJ),
                ("gravity", ctypes.c_double * 3), ("algorithm", ctypes.c_int), ("floating_base", ctypes.c_int),
                ("nspheres", ctypes.c_int), ("sphere_link", ctypes.c_int * _NS), ("sphere_center", (ctypes.c_double * 3) * _NS),
                ("sphere_radius", ctypes.c_double * _NS), ("plane_R", ctypes.c_double * 9), ("plane_o", ctypes.c_double * 3),
                ("cp_epsilon", ctypes.c_double), ("cp_mu_coulomb", ctypes.c_double), ("min_step_size", ctypes.c_double),
                ("contact_dist_thresh", ctypes.c_double), ("cp_mu_viscous", ctypes.c_double), ("cp_compliance", ctypes.c_double),
                ("cp_nk", ctypes.c_int), ("cstab_max_iterations", ctypes.c_int), ("cstab_eps", ctypes.c_double),
                ("nboxes", ctypes.c_int), ("box_link", ctypes.c_int * _NB), ("box_center", (ctypes.c_double * 3) * _NB),
                ("box_R", (ctypes.c_double * 9) * _NB), ("box_len", (ctypes.c_double * 3) * _NB),
                ("npairs", ctypes.c_int), ("pair_a", ctypes.c_int * _NP), ("pair_b", ctypes.c_int * _NP), ("sphere_no_plane", ctypes.c_int),
                ("pair_kind", ctypes.c_int * _NP)]


MH_ARTIC_CRB, MH_ARTIC_FSAB = 0, 1      # moby_hip_artic.h: RCArticulatedBody::algorithm_type
MH_DRIVE_FORCE, MH_DRIVE_PD = 1, 2       # moby_hip_artic.h: mh_artic_drive.terms
MH_ARTIC_BASE_ANGLES, MH_ARTIC_BASE_POSE = 0, 1     # moby_hip_artic.h: mh_artic_batch_set_base_coords
_BASE_COORDS = {"angles": MH_ARTIC_BASE_ANGLES, "pose": MH_ARTIC_BASE_POSE}
REPORT_PAIR = 8      # MH_REPORT_PAIR: doubles per (world, step, slot) row of the contact report (include/moby_hip_artic.h, "Contact report")


def report_slots(model):
    """nspheres + nboxes + npairs: the slots of the model's contact report (mh_artic_report_slots; host only)"""
    n = _lib.load().mh_artic_report_slots(ctypes.byref(model))
    if n < 0:
        _lib.check(n)
    return n


def link_impulses(report, model):
    """The net linear contact impulse on every link from rows of the contact report: (..., nslots, 8) -> (..., nj, 3), model-frame axes.  Entries
    [2..4] of a slot's row are the impulse on the reference's geometry A: the link of a sphere or box on the plane, pair_a's link for a pair, whose
    other link (pair_b's sphere) received the negative.  A static box (link -1) is skipped.  numpy arrays and torch tensors alike."""
    ns, nb = model.nspheres, model.nboxes
    assert report.shape[-2:] == (ns + nb + model.npairs, REPORT_PAIR), report.shape
    out = (report.new_zeros if _is_tensor(report) else lambda sh: np.zeros(sh, dtype=report.dtype))(tuple(report.shape[:-2]) + (model.nj, 3))
    terms = [(s, model.sphere_link[s], None) for s in range(ns)] + [(ns + b, model.box_link[b], None) for b in range(nb)]
    for k in range(model.npairs):
        a = model.box_link[model.pair_a[k]] if model.pair_kind[k] == MH_ARTIC_PAIR_BOX_SPHERE else model.sphere_link[model.pair_a[k]]
        terms.append((ns + nb + k, a, model.sphere_link[model.pair_b[k]]))
    for slot, la, lb in terms:
        jv = report[..., slot, 2:5]
        if la >= 0:
            out[..., la, :] += jv
        if lb is not None:
            out[..., lb, :] -= jv
    return out


_D = ctypes.c_double


class mh_artic_params(ctypes.Structure):
    """One world's values of the shared model (include/moby_hip_artic.h, "Per-world parameters"): doubles only, the model's indexing"""
    _fields_ = [("Rrel", (_D * 9) * _NJ), ("trel", (_D * 3) * _NJ), ("axis", (_D * 3) * _NJ), ("com", (_D * 3) * _NJ), ("inertia", (_D * 9) * _NJ),
                ("mass", _D * _NJ), ("lolimit", _D * _NJ), ("hilimit", _D * _NJ), ("limit_restitution", _D * _NJ), ("gravity", _D * 3),
                ("sphere_center", (_D * 3) * _NS), ("sphere_radius", _D * _NS), ("plane_R", _D * 9), ("plane_o", _D * 3),
                ("cp_epsilon", _D), ("cp_mu_coulomb", _D), ("cp_mu_viscous", _D), ("cp_compliance", _D),
                ("box_center", (_D * 3) * _NB), ("box_R", (_D * 9) * _NB), ("box_len", (_D * 3) * _NB)]


# the same layout as a numpy record: params["mass"][w, i], params["box_len"][w, k, c], params["cp_mu_coulomb"][w]
PARAMS_DTYPE = np.dtype([("Rrel", "f8", (_NJ, 9)), ("trel", "f8", (_NJ, 3)), ("axis", "f8", (_NJ, 3)), ("com", "f8", (_NJ, 3)), ("inertia", "f8", (_NJ, 9)),
                         ("mass", "f8", (_NJ,)), ("lolimit", "f8", (_NJ,)), ("hilimit", "f8", (_NJ,)), ("limit_restitution", "f8", (_NJ,)), ("gravity", "f8", (3,)),
                         ("sphere_center", "f8", (_NS, 3)), ("sphere_radius", "f8", (_NS,)), ("plane_R", "f8", (9,)), ("plane_o", "f8", (3,)),
                         ("cp_epsilon", "f8"), ("cp_mu_coulomb", "f8"), ("cp_mu_viscous", "f8"), ("cp_compliance", "f8"),
                         ("box_center", "f8", (_NB, 3)), ("box_R", "f8", (_NB, 9)), ("box_len", "f8", (_NB, 3))])
PARAMS_DOUBLES = PARAMS_DTYPE.itemsize // 8      # a record as a row of doubles (a (count, PARAMS_DOUBLES) tensor for set_params_dev)
MH_ARTIC_CREATE_REPORT = 1


def make_params(model, B):
    """B records, every one equal to the model (what mh_artic_params_from_model writes): the array to vary and hand to ArticBatch(params=...)"""
    p = np.zeros(B, dtype=PARAMS_DTYPE)
    for name in PARAMS_DTYPE.names:
        p[name] = np.array(getattr(model, name), dtype=np.float64).reshape(PARAMS_DTYPE[name].shape)
    return p


def _records(params, count=None):
    p = np.ascontiguousarray(params)
    if p.dtype != PARAMS_DTYPE or p.ndim != 1 or (count is not None and p.shape[0] != count):
        raise ValueError("expected %s records of artic.PARAMS_DTYPE (artic.make_params), got %r %r" % ("" if count is None else count, p.dtype, p.shape))
    return p


class mh_artic_drive(ctypes.Structure):
    _fields_ = [("terms", ctypes.c_int), ("rows", ctypes.c_int), ("kp", ctypes.c_void_p), ("kv", ctypes.c_void_p),
                ("q_des", ctypes.c_void_p), ("qd_des", ctypes.c_void_p), ("tau_ff", ctypes.c_void_p)]


class Drive:
    """Joint forces and PD joint servos evaluated inside the step, once per mini-step (include/moby_hip_artic.h, mh_artic_drive):
        tau = (kp * (q_des - q) + kv * (qd_des - qd)) + tau_ff
    PD (kp, kv, q_des, qd_des: all four or none) and the feed-forward force tau_ff are independent terms; an absent term is not in the sum.
    kp, kv: (B, nj).  q_des, qd_des, tau_ff: (B, nj) held for the whole launch, or (R, B, nj) schedules whose row s drives step s of the
    launch (R >= nsteps).  Arrays are numpy (staged to the device) or float64 contiguous torch tensors on the batch's device (zero-copy)."""
    _PD = ("kp", "kv", "q_des", "qd_des")
    _SCHED = ("q_des", "qd_des", "tau_ff")

    def __init__(self, kp=None, kv=None, q_des=None, qd_des=None, tau_ff=None):
        self.arrays = dict(kp=kp, kv=kv, q_des=q_des, qd_des=qd_des, tau_ff=tau_ff)
        given = [self.arrays[k] is not None for k in self._PD]
        if any(given) and not all(given):
            raise ValueError("Drive: PD needs kp, kv, q_des and qd_des")
        self.terms = (MH_DRIVE_PD if all(given) else 0) | (MH_DRIVE_FORCE if tau_ff is not None else 0)
        shapes = {k: tuple(a.shape) for k, a in self.arrays.items() if a is not None}
        sched = {shapes[k][0] if len(shapes[k]) == 3 else 1 for k in self._SCHED if k in shapes}
        if len(sched) > 1:
            raise ValueError("Drive: q_des, qd_des and tau_ff must have the same number of schedule rows: %r" % shapes)
        self.rows = sched.pop() if sched else 1
        self.shapes = shapes

    def check(self, B, nj):
        for k, sh in self.shapes.items():
            want = [(B, nj)] + ([(self.rows, B, nj)] if k in self._SCHED else [])
            if sh not in want:
                raise ValueError("Drive.%s: shape %r, expected %s" % (k, sh, " or ".join(map(str, want))))


def _is_tensor(a):
    return type(a).__module__.startswith("torch")


MH_LINK_WRENCH, MH_LINK_DAMPING, MH_LINK_WRENCH_LINK_AXES = 1, 2, 4


class mh_artic_wrench(ctypes.Structure):
    _fields_ = [("terms", ctypes.c_int), ("rows", ctypes.c_int), ("w", ctypes.c_void_p), ("kl", ctypes.c_void_p), ("ka", ctypes.c_void_p),
                ("klsq", ctypes.c_void_p), ("kasq", ctypes.c_void_p)]


class LinkWrench:
    """Forces on links evaluated inside the step, once per mini-step (include/moby_hip_artic.h, "Link wrenches", mh_artic_wrench).
    w: (B, nj, 6) held for the whole launch, or (R, B, nj, 6) whose row s acts during step s (R >= nsteps): fx fy fz at the link's COM and a free
    torque nx ny nz, in model axes, or in the link's own axes with link_axes=True.  kl, ka, klsq, kasq: (B, nj) each, all four or none -- the
    links' linear, angular and quadratic damping.  The terms are independent; an absent one is not in the sum.  float64 contiguous torch tensors
    on the batch's device, for a batch created with wrench=True."""
    _DAMP = ("kl", "ka", "klsq", "kasq")

    def __init__(self, w=None, kl=None, ka=None, klsq=None, kasq=None, link_axes=False):
        self.arrays = dict(w=w, kl=kl, ka=ka, klsq=klsq, kasq=kasq)
        given = [self.arrays[k] is not None for k in self._DAMP]
        if any(given) and not all(given):
            raise ValueError("LinkWrench: damping needs kl, ka, klsq and kasq")
        if link_axes and w is None:
            raise ValueError("LinkWrench: link_axes without w")
        self.terms = (MH_LINK_WRENCH if w is not None else 0) | (MH_LINK_DAMPING if all(given) else 0) | (MH_LINK_WRENCH_LINK_AXES if link_axes else 0)
        self.shapes = {k: tuple(a.shape) for k, a in self.arrays.items() if a is not None}
        self.rows = self.shapes["w"][0] if len(self.shapes.get("w", ())) == 4 else 1

    def check(self, B, nj, nsteps):
        for k, sh in self.shapes.items():
            want = [(B, nj, 6), (self.rows, B, nj, 6)] if k == "w" else [(B, nj)]
            if sh not in want:
                raise ValueError("LinkWrench.%s: shape %r, expected %s" % (k, sh, " or ".join(map(str, want))))
        if 1 < self.rows < nsteps:
            raise ValueError("LinkWrench.w: %d schedule rows for %d steps (one held row, or at least one per step)" % (self.rows, nsteps))


class mh_io_artic(ctypes.Structure):
    _fields_ = [("model", mh_artic_model), ("link_id", (ctypes.c_char * mio.MH_IO_ID_LEN) * _NJ),
                ("joint_id", (ctypes.c_char * mio.MH_IO_ID_LEN) * _NJ)]


def load_sdf(path, gravity=(0.0, 0.0, -9.81)):
    """-> (mh_artic_model, link names, joint names): SDFReader::read_model's articulated-body branch (SDFReader.cpp:928-996)."""
    lib = mio.load()
    lib.mh_io_load_sdf.restype = ctypes.c_int
    lib.mh_io_load_sdf.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(mh_io_artic)]
    io = mh_io_artic()
    g = (ctypes.c_double * 3)(*gravity)
    if lib.mh_io_load_sdf(os.fsencode(path), g, ctypes.byref(io)) != 0:
        raise mio.SceneError(lib.mh_io_last_error().decode("utf-8", "replace"))
    m = mh_artic_model()
    ctypes.memmove(ctypes.addressof(m), ctypes.addressof(io.model), ctypes.sizeof(mh_artic_model))
    return m, [io.link_id[i].value.decode() for i in range(m.nj)], [io.joint_id[i].value.decode() for i in range(m.nj)]


def load_urdf(path, gravity=(0.0, 0.0, -9.81)):
    """A URDF robot with a fixed base (src/URDFReader.cpp; include/moby_hip_io.h: mh_io_load_urdf) -> (model, link ids, joint ids)."""
    lib = mio.load()
    lib.mh_io_load_urdf.restype = ctypes.c_int
    lib.mh_io_load_urdf.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(mh_io_artic)]
    out = mh_io_artic()
    g = (ctypes.c_double * 3)(*gravity)
    if lib.mh_io_load_urdf(os.fsencode(path), g, ctypes.byref(out)) != 0:
        raise mio.SceneError(lib.mh_io_last_error().decode("utf-8", "replace"))
    m = mh_artic_model()
    ctypes.memmove(ctypes.addressof(m), ctypes.addressof(out.model), ctypes.sizeof(mh_artic_model))
    return m, [out.link_id[i].value.decode() for i in range(m.nj)], [out.joint_id[i].value.decode() for i in range(m.nj)]


def load_xml(path):
    """-> (mh_artic_model, link names, joint names, q0, qd0, step size): a Moby XML file with one RCArticulatedBody (fixed base, or floating-base="true": six virtual joints first, include/moby_hip_io.h)
    (include/moby_hip_io.h: mh_io_load_xml_artic) -- the model at q = 0, the joints' q / qd attributes as the initial state."""
    lib = mio.load()
    lib.mh_io_load_xml_artic.restype = ctypes.c_int
    lib.mh_io_load_xml_artic.argtypes = [ctypes.c_char_p, ctypes.POINTER(mh_io_artic), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_double)]
    io = mh_io_artic(); q0 = (ctypes.c_double * _NJ)(); qd0 = (ctypes.c_double * _NJ)(); dt = ctypes.c_double(0.0)
    if lib.mh_io_load_xml_artic(os.fsencode(path), ctypes.byref(io), q0, qd0, ctypes.byref(dt)) != 0:
        raise mio.SceneError(lib.mh_io_last_error().decode("utf-8", "replace"))
    m = mh_artic_model()
    ctypes.memmove(ctypes.addressof(m), ctypes.addressof(io.model), ctypes.sizeof(mh_artic_model))
    n = m.nj
    return (m, [io.link_id[i].value.decode() for i in range(n)], [io.joint_id[i].value.decode() for i in range(n)],
            np.array(q0[:n]), np.array(qd0[:n]), dt.value)


def model_from_links(links, gravity=(0.0, 0.0, -9.81), floating_base=None):
    """links: dicts (parents first) with parent (-1 = base), type, R0 (3x3, model frame at q = 0), x0, axis (model frame),
    com (link frame), inertia (3x3 about the COM, link axes), mass, lo, hi, restitution.
    floating_base = dict(R0, x0, mass, inertia): the base link (pose of its COM frame in the global frame, inertia in its own axes) is carried by the six
    virtual joints of mh_artic_model.floating_base (include/moby_hip_artic.h) -- joints 0..5 of the returned model, the base link is link 5, `links` follow
    as joints 6.. with parent -1 meaning the base link; exactly what mh_io_load_xml_artic builds for floating-base="true"."""
    if floating_base is not None:
        Rb = np.asarray(floating_base["R0"], dtype=float); xb = np.asarray(floating_base["x0"], dtype=float)
        virt = [dict(parent=v - 1, type=MH_JOINT_PRISMATIC if v < 3 else MH_JOINT_REVOLUTE, R0=np.eye(3) if v < 3 else Rb, x0=xb,
                     axis=(np.eye(3) if v < 3 else Rb)[:, v % 3], com=(0.0, 0.0, 0.0), inertia=floating_base["inertia"] if v == 5 else np.zeros((3, 3)),
                     mass=float(floating_base["mass"]) if v == 5 else 0.0) for v in range(6)]
        links = virt + [dict(L, parent=5 if L["parent"] < 0 else L["parent"] + 6) for L in links]
    m = mh_artic_model()
    m.nj = len(links)
    for i, L in enumerate(links):
        p = L["parent"]
        Rp = np.eye(3) if p < 0 else np.asarray(links[p]["R0"], dtype=float)
        xp = np.zeros(3) if p < 0 else np.asarray(links[p]["x0"], dtype=float)
        Rc = np.asarray(L["R0"], dtype=float); xc = np.asarray(L["x0"], dtype=float)
        Rrel = Rp.T @ Rc; trel = Rp.T @ (xc - xp)
        al = Rc.T @ np.asarray(L["axis"], dtype=float); al = al / np.linalg.norm(al)
        m.parent[i] = p; m.jtype[i] = L.get("type", MH_JOINT_REVOLUTE)
        for k in range(9):
            m.Rrel[i][k] = Rrel.flat[k]; m.inertia[i][k] = np.asarray(L["inertia"], dtype=float).flat[k]
        for k in range(3):
            m.trel[i][k] = trel[k]; m.axis[i][k] = al[k]; m.com[i][k] = L["com"][k]
        m.mass[i] = L["mass"]
        m.lolimit[i] = L.get("lo", -np.finfo(float).max); m.hilimit[i] = L.get("hi", np.finfo(float).max)
        m.limit_restitution[i] = L.get("restitution", 0.0)
    for k in range(3):
        m.gravity[k] = gravity[k]
    if floating_base is not None:          # the layout mh_artic_batch_create checks, free of the round-off of Rb' Rb
        m.floating_base = 1
        for v in range(6):
            for k in range(3):
                m.axis[v][k] = float(k == v % 3)
                if v > 0: m.trel[v][k] = 0.0
            if v != 3:
                for k in range(9): m.Rrel[v][k] = float(k % 4 == 0)
    m.cstab_eps = S.NEAR_ZERO              # ConstraintStabilization::eps (CStab:59); stabilisation itself off until cstab_max_iterations is set
    return m


def add_spheres(model, spheres, plane_normal=(0.0, 0.0, 1.0), plane_point=(0.0, 0.0, 0.0), epsilon=0.0, mu_coulomb=100.0, mu_viscous=0.0,
                compliance=0.0, nk=4):
    """Sphere primitives on links against one static plane: spheres = [(link, centre in the link frame, radius), ...]; the
    plane through plane_point with the given normal (the +Y axis of the plane frame, as PlanePrimitive has it); the
    ContactParameters of the (robot, plane) pair (ur10.xml:19: epsilon 0, mu-coulomb 100).  Returns the model."""
    assert 0 < len(spheres) <= MH_ARTIC_MAX_SPHERES
    Rp = _plane_frame(model, plane_normal, plane_point, model.nboxes > 0)
    model.nspheres = len(spheres)
    for i, (link, c, r) in enumerate(spheres):
        assert 0 <= link < model.nj and r > 0
        model.sphere_link[i] = int(link); model.sphere_radius[i] = float(r)
        for k in range(3):
            model.sphere_center[i][k] = float(c[k])
    _set_plane(model, Rp, plane_point, epsilon, mu_coulomb, mu_viscous, compliance, nk)
    return model


def _plane_frame(model, plane_normal, plane_point, shared):
    """The plane frame of a normal (its +Y axis); shared: the model's other kind of primitive already has a plane -- refuse one that disagrees."""
    n = np.asarray(plane_normal, dtype=float); n = n / np.linalg.norm(n)
    e = np.eye(3)[int(np.argmin(np.abs(n)))]
    xax = np.cross(n, e); xax = xax / np.linalg.norm(xax); zax = np.cross(xax, n)
    Rp = np.column_stack([xax, n, zax])                       # columns: the plane frame's axes; +Y = normal
    if shared:
        if list(Rp.flat) != list(model.plane_R) or [float(v) for v in plane_point] != list(model.plane_o):
            raise ValueError("the model's spheres and boxes share one plane: this one disagrees with the plane already set")
    return Rp


def _set_plane(model, Rp, plane_point, epsilon, mu_coulomb, mu_viscous, compliance, nk):
    for k in range(9):
        model.plane_R[k] = Rp.flat[k]
    for k in range(3):
        model.plane_o[k] = float(plane_point[k])
    model.cp_epsilon = float(epsilon); model.cp_mu_coulomb = float(mu_coulomb)
    model.cp_mu_viscous = float(mu_viscous); model.cp_compliance = float(compliance); model.cp_nk = int(nk)
    model.min_step_size = S.NEAR_ZERO
    model.contact_dist_thresh = 1e-6


def add_boxes(model, boxes, plane_normal=(0.0, 0.0, 1.0), plane_point=(0.0, 0.0, 0.0), epsilon=0.0, mu_coulomb=100.0, mu_viscous=0.0,
              compliance=0.0, nk=4):
    """Box primitives on links against the model's one static plane (include/moby_hip_artic.h, mh_artic_model.nboxes):
    boxes = [(link, centre in the link frame, R (the box's axes in the link frame, 3x3), (xlen, ylen, zlen) full edge lengths), ...].
    link = -1 is a static box: centre and R are its pose in the model frame; it never meets the plane and must appear in a box-sphere pair
    (add_box_sphere_pairs).
    The plane and the ContactParameters are those of add_spheres, shared with the spheres (one set per model: the last call sets the
    parameters; a plane that disagrees with one already set is refused).  Returns the model."""
    assert 0 < len(boxes) <= MH_ARTIC_MAX_BOXES
    Rp = _plane_frame(model, plane_normal, plane_point, model.nspheres > 0)
    model.nboxes = len(boxes)
    for i, (link, c, R, dims) in enumerate(boxes):
        R = np.asarray(R, dtype=float).reshape(3, 3)
        assert -1 <= link < model.nj and all(d > 0 for d in dims)
        model.box_link[i] = int(link)
        for k in range(3):
            model.box_center[i][k] = float(c[k]); model.box_len[i][k] = float(dims[k])
        for k in range(9):
            model.box_R[i][k] = R.flat[k]
    _set_plane(model, Rp, plane_point, epsilon, mu_coulomb, mu_viscous, compliance, nk)
    return model


def add_pairs(model, pairs, no_plane=()):
    """Sphere contacts between links (include/moby_hip_artic.h, mh_artic_model.npairs): pairs = [(a, b), ...] name two spheres of the model's
    sphere list (add_spheres first) that sit on different links -- a is the reference's geometry A, the contact normal points from b to a;
    no_plane lists the spheres that do not meet the plane.  The pairs share the model's contact parameters with the plane contacts.
    mh_artic_batch_create checks the rest (indices, a pair listed twice).  Returns the model."""
    assert len(pairs) <= MH_ARTIC_MAX_PAIRS
    model.npairs = len(pairs)
    for k, (a, b) in enumerate(pairs):
        model.pair_a[k] = int(a); model.pair_b[k] = int(b); model.pair_kind[k] = MH_ARTIC_PAIR_SPHERES
    mask = 0
    for s in no_plane:
        assert 0 <= int(s) < MH_ARTIC_MAX_SPHERES
        mask |= 1 << int(s)
    model.sphere_no_plane = mask
    return model


def add_box_sphere_pairs(model, pairs, no_plane=()):
    """Box-sphere contacts between links (include/moby_hip_artic.h, mh_artic_model.pair_kind): pairs = [(box, sphere), ...] name a box of the
    model's box list (add_boxes first; a static box has link -1) and a sphere of its sphere list on a different link.  The box is the reference's
    geometry A.  APPENDS to the pairs already set (add_pairs before it); no_plane lists further spheres that do not meet the plane.
    mh_artic_batch_create checks the rest.  Returns the model."""
    assert model.npairs + len(pairs) <= MH_ARTIC_MAX_PAIRS
    for box, sph in pairs:
        k = model.npairs
        model.pair_a[k] = int(box); model.pair_b[k] = int(sph); model.pair_kind[k] = MH_ARTIC_PAIR_BOX_SPHERE
        model.npairs = k + 1
    for s in no_plane:
        assert 0 <= int(s) < MH_ARTIC_MAX_SPHERES
        model.sphere_no_plane |= 1 << int(s)
    return model


def chain_model(n, length=0.5, mass=1.0, lo=-1.0, hi=1.0, restitution=0.0, gravity=(0.0, 0.0, -9.81), prismatic_last=False):
    """n rods hanging along -z from the origin, hinged about y (a planar n-pendulum); optionally the last joint slides."""
    links = []
    for i in range(n):
        I = mass * length * length / 12.0
        links.append(dict(parent=i - 1, type=MH_JOINT_PRISMATIC if (prismatic_last and i == n - 1) else MH_JOINT_REVOLUTE,
                          R0=np.eye(3), x0=(0.0, 0.0, -length * i), axis=(0.0, 0.0, 1.0) if (prismatic_last and i == n - 1) else (0.0, 1.0, 0.0),
                          com=(0.0, 0.0, -0.5 * length), inertia=np.diag([I, I, 1e-3 * I]), mass=mass, lo=lo, hi=hi, restitution=restitution))
    return model_from_links(links, gravity)


class ArticBatch:
    """B worlds of one articulated body on the GPU.  base_coords ("angles", the default, or "pose"): how a floating base's configuration is
    carried -- three Euler-like angles in the virtual joints, or a per-world pose (p, Q) the virtual joints are folded into after every step
    (include/moby_hip_artic.h, MH_ARTIC_BASE_POSE: no singularity at a quarter turn of the middle hinge).  "pose" folds q / qd as given."""

    def __init__(self, model, q, qd, aux=None, base_coords="angles", report=False, params=None, wrench=False):
        """wrench=True: a batch of mh_artic_batch_create_wrench -- a params batch (records from params=, or all equal to the model) that also takes
        step(..., wrench=LinkWrench(...)) (include/moby_hip_artic.h, "Link wrenches").
        params: B records of PARAMS_DTYPE (make_params), one per world, or True for records that all equal the model -- a batch of
        mh_artic_batch_create_params: world w steps the model with record w written into it (include/moby_hip_artic.h, "Per-world parameters");
        set_params / set_params_dev replace records later.
        report=True: a batch of mh_artic_batch_create_report -- it steps through the report kernels and step(..., report=tensor) fills the
        per-slot contact impulse report (include/moby_hip_artic.h, "Contact report")"""
        lib = _lib.load()
        self.model = model
        self.nj = model.nj
        q = np.ascontiguousarray(q, dtype=np.float64); qd = np.ascontiguousarray(qd, dtype=np.float64)
        self.B = q.shape[0]
        assert q.shape == (self.B, self.nj) and qd.shape == q.shape
        self.handle = ctypes.c_void_p()
        self._staged = None
        self.report = bool(report)
        self.wrench = bool(wrench)
        self.params = params is not None or self.wrench
        if self.params:
            p = None if params is True or params is None else _records(params, self.B)
            _lib.check((lib.mh_artic_batch_create_wrench if self.wrench else lib.mh_artic_batch_create_params)(ctypes.byref(model), None if p is None else p.ctypes.data, self.B, MH_ARTIC_CREATE_REPORT if report else 0, ctypes.byref(self.handle)))
        else:
            _lib.check((lib.mh_artic_batch_create_report if report else lib.mh_artic_batch_create)(ctypes.byref(model), self.B, ctypes.byref(self.handle)))
        self.report_slots = report_slots(model)
        self.upload(q, qd, aux)
        if base_coords != "angles":
            self.set_base_coords(base_coords)

    def set_params(self, records, first=0):
        """Replace the records of worlds first .. first + len(records) - 1 (PARAMS_DTYPE), validated as at create; synchronous.  A refused record
        leaves every world as it was."""
        p = _records(records)
        _lib.check(_lib.load().mh_artic_batch_set_params(self.handle, p.ctypes.data, int(first), int(p.shape[0])))

    def set_params_dev(self, records_t, first=0, stream=None):
        """The same from a float64 contiguous (count, PARAMS_DOUBLES) torch tensor on the batch's device -- record rows laid out as PARAMS_DTYPE --
        scattered by a kernel on `stream`, in order with the launches of that stream.  NOT validated (include/moby_hip_artic.h says what a bad
        value does)."""
        import torch
        if records_t.dtype != torch.float64 or records_t.dim() != 2:
            raise ValueError("expected a contiguous float64 tensor of shape (count, %d) on %s, got %s %r on %s" % (PARAMS_DOUBLES, self._device(), records_t.dtype, tuple(records_t.shape), records_t.device))
        _lib.check(_lib.load().mh_artic_batch_set_params_dev(self.handle, stream, self._tensor_ptr(records_t, (records_t.shape[0], PARAMS_DOUBLES)), int(first), int(records_t.shape[0])))

    def set_base_coords(self, coords):
        """"pose" (or MH_ARTIC_BASE_POSE): switch to pose coordinates -- every world's pose from the model, the resident q / qd folded into it.
        Floating bases without finite limits on the virtual joints only; there is no way back to angles."""
        c = _BASE_COORDS.get(coords, coords)
        _lib.check(_lib.load().mh_artic_batch_set_base_coords(self.handle, int(c)))

    @property
    def base_coords(self):
        c = ctypes.c_int(-1)
        _lib.check(_lib.load().mh_artic_batch_base_coords(self.handle, ctypes.byref(c)))
        return {v: k for k, v in _BASE_COORDS.items()}[c.value]

    def base_pose(self):
        """(B, 7): px py pz (the base COM, model frame), qw qx qy qz (unit quaternion of the base's orientation); pose coordinates only"""
        P = np.zeros((self.B, 7))
        _lib.check(_lib.load().mh_artic_batch_base_pose(self.handle, P.ctypes.data))
        return P

    def set_base_pose(self, pose):
        """(B, 7) as base_pose returns it; each quaternion is normalised, a zero or non-finite one refused.  With download / upload this is a
        pose batch's checkpoint / restore."""
        P = np.ascontiguousarray(pose, dtype=np.float64); assert P.shape == (self.B, 7)
        _lib.check(_lib.load().mh_artic_batch_set_base_pose(self.handle, P.ctypes.data))

    def base_pose_into(self, pose_t, stream=None):
        """The poses into a float64 contiguous (B, 7) torch tensor on the batch's device, stream-ordered (no host sync)."""
        _lib.check(_lib.load().mh_artic_batch_base_pose_dev(self.handle, stream, self._tensor_ptr(pose_t, (self.B, 7))))

    def upload(self, q=None, qd=None, aux=None):
        P = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data
        _lib.check(_lib.load().mh_artic_batch_upload(self.handle, P(q), P(qd), P(aux)))

    def _device(self):
        import torch
        return torch.device("cuda", _lib.load().mh_artic_batch_device(self.handle))

    def _tensor_ptr(self, t, shape, dtype=None):
        """dtype: the tensor's torch dtype (None = torch.float64)"""
        import torch
        dtype = torch.float64 if dtype is None else dtype
        if t.dtype != dtype or not t.is_contiguous() or t.device != self._device() or tuple(t.shape) != tuple(shape):
            raise ValueError("expected a contiguous %s tensor of shape %r on %s, got %s %r on %s" % (str(dtype).replace("torch.", ""), tuple(shape), self._device(), t.dtype, tuple(t.shape), t.device))
        return t.data_ptr()

    def reset(self, mask=None, q=None, qd=None, pose=None, stream=None):
        """A new episode in some worlds, on `stream`, with no host synchronisation (mh_artic_batch_reset_dev; include/moby_hip_artic.h, "Episodes on
        the device").  mask: a contiguous torch.int32 (B,) tensor on the batch's device, world w is reset iff mask[w] != 0; None = every world.
        q, qd: float64 (B, nj); pose: float64 (B, 7), pose coordinates only -- only the rows of reset worlds are read, None leaves that array as it
        is.  A reset world's aux record becomes a fresh one (rand() at srand(1), time, status, warm starts and counters 0) whatever was given; a
        world that is not reset is not touched.  The values are NOT validated."""
        import torch
        if mask is not None and (not _is_tensor(mask) or mask.dtype != torch.int32):
            raise ValueError("reset: mask must be a torch.int32 tensor of shape (%d,) on the batch's device, got %s -- convert it (torch.as_tensor(done, dtype=torch.int32, device=...))"
                             % (self.B, mask.dtype if _is_tensor(mask) else type(mask).__name__))
        P = lambda t, shape: None if t is None else self._tensor_ptr(t, shape)
        mp = None if mask is None else self._tensor_ptr(mask, (self.B,), torch.int32)
        _lib.check(_lib.load().mh_artic_batch_reset_dev(self.handle, stream, mp, P(q, (self.B, self.nj)), P(qd, (self.B, self.nj)), P(pose, (self.B, 7))))

    def status_into(self, status_t=None, time_t=None, stream=None):
        """Every world's status bits into an int32 (B,) tensor and its time into a float64 (B,) tensor on the batch's device (either may be None, not
        both), stream-ordered (no host sync): which worlds have ended."""
        import torch
        sp = None if status_t is None else self._tensor_ptr(status_t, (self.B,), torch.int32)
        tp = None if time_t is None else self._tensor_ptr(time_t, (self.B,))
        _lib.check(_lib.load().mh_artic_batch_status_dev(self.handle, stream, sp, tp))

    def link_poses_into(self, poses_t, stream=None):
        """link_poses() into a float64 contiguous (B, nj, 12) torch tensor on the batch's device, stream-ordered (no host sync, no allocation): the
        same kernels, bit-equal to the host call."""
        _lib.check(_lib.load().mh_artic_batch_link_poses_dev(self.handle, stream, self._tensor_ptr(poses_t, (self.B, self.nj, 12))))

    def step(self, dt, nsteps=1, stream=None, drive=None, report=None, wrench=None):
        """nsteps x TimeSteppingSimulator::step(dt) in one launch on `stream` (a raw HIP stream handle; None = the null stream).
        drive: a Drive for this launch; None = the drive stored by set_drive (none: undriven).  A torch loop passes
        torch.cuda.current_stream().cuda_stream here and to state_into, so that both run in order with its own kernels.
        report: a float64 contiguous (B, nsteps, report_slots, 8) torch tensor on the batch's device that receives the launch's contact report
        (a batch created with report=True only); None = nothing is written.
        wrench: a LinkWrench of device tensors for this launch (a batch created with wrench=True only); None = no force on the links."""
        lib = _lib.load()
        rp = None
        if report is not None:
            if not self.report:
                raise ValueError("a report needs a batch created with report=True")
            rp = self._tensor_ptr(report, (self.B, int(nsteps), self.report_slots, REPORT_PAIR))
        if self._staged is not None:               # numpy arrays staged by the previous launch: free them once it has read them
            import torch
            torch.cuda.synchronize(self._device())
            self._staged = None
        d = None
        if drive is not None:
            drive.check(self.B, self.nj)
            d = mh_artic_drive(terms=drive.terms, rows=drive.rows)
            staged = []
            for k, a in drive.arrays.items():
                if a is None:
                    continue
                if not _is_tensor(a):
                    import torch
                    a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self._device())
                    staged.append(a)
                setattr(d, k, self._tensor_ptr(a, a.shape))
            self._staged = staged or None
        if wrench is not None:
            if not self.wrench:
                raise ValueError("a wrench needs a batch created with wrench=True")
            wrench.check(self.B, self.nj, int(nsteps))
            w = mh_artic_wrench(terms=wrench.terms, rows=wrench.rows)
            for k, a in wrench.arrays.items():
                if a is not None:
                    setattr(w, k, self._tensor_ptr(a, a.shape))
            _lib.check(lib.mh_artic_batch_step_wrench(self.handle, stream, float(dt), int(nsteps), None if d is None else ctypes.byref(d), ctypes.byref(w), rp))
        elif self.report:
            _lib.check(lib.mh_artic_batch_step_report(self.handle, stream, float(dt), int(nsteps), None if d is None else ctypes.byref(d), rp))
        else:
            _lib.check(lib.mh_artic_batch_step_driven(self.handle, stream, float(dt), int(nsteps), None if d is None else ctypes.byref(d)))

    def set_drive(self, drive=None):
        """Store a Drive (host copies of its arrays on the device) for every later step(..., drive=None); None clears it."""
        if drive is None:
            _lib.check(_lib.load().mh_artic_batch_set_drive(self.handle, None))
            return
        drive.check(self.B, self.nj)
        d = mh_artic_drive(terms=drive.terms, rows=drive.rows)
        keep = []
        for k, a in drive.arrays.items():
            if a is None:
                continue
            h = np.ascontiguousarray(a.detach().cpu().numpy() if _is_tensor(a) else a, dtype=np.float64)
            keep.append(h)
            setattr(d, k, h.ctypes.data)
        _lib.check(_lib.load().mh_artic_batch_set_drive(self.handle, ctypes.byref(d)))

    def state_into(self, q_t=None, qd_t=None, stream=None):
        """The resident q / qd into float64 contiguous (B, nj) torch tensors on the batch's device, stream-ordered (no host sync)."""
        P = lambda t: None if t is None else self._tensor_ptr(t, (self.B, self.nj))
        _lib.check(_lib.load().mh_artic_batch_state_dev(self.handle, stream, P(q_t), P(qd_t)))

    def fwd_dyn(self, tau=None, want_H=True):
        qdd = np.zeros((self.B, self.nj)); H = np.zeros((self.B, self.nj, self.nj)) if want_H else None
        t = None if tau is None else np.ascontiguousarray(tau, dtype=np.float64)
        _lib.check(_lib.load().mh_artic_batch_fwd_dyn(self.handle, None if t is None else t.ctypes.data, qdd.ctypes.data,
                                                      None if H is None else H.ctypes.data))
        return qdd, H

    def link_poses(self):
        P = np.zeros((self.B, self.nj, 12))
        _lib.check(_lib.load().mh_artic_batch_link_poses(self.handle, P.ctypes.data))
        return P

    def jacobian(self, link, points):
        """calc_jacobian for every resident state: (B, 6, nj); points (B, 3) in the model frame."""
        p = np.ascontiguousarray(points, dtype=np.float64); assert p.shape == (self.B, 3)
        J = np.zeros((self.B, 6, self.nj))
        _lib.check(_lib.load().mh_artic_batch_jacobian(self.handle, int(link), p.ctypes.data, J.ctypes.data))
        return J

    def download(self):
        q = np.zeros((self.B, self.nj)); qd = np.zeros((self.B, self.nj)); aux = np.zeros(self.B, dtype=S.AUX_DTYPE)
        _lib.check(_lib.load().mh_artic_batch_download(self.handle, q.ctypes.data, qd.ctypes.data, aux.ctypes.data))
        return q, qd, aux

    def close(self):
        if self.handle:
            _lib.load().mh_artic_batch_destroy(self.handle)
            self.handle = None
        self._staged = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
