"""The hanging garment: a cloth of point masses and distance constraints under gravity, held at one vertex, stepped with small-step XPBD.  It makes
mesh/cloth_verts of a dataset store from the canonical mesh (mesh/cloth_nocs_verts, mesh/cloth_faces_tri): the one array every derived group starts from.

Definition (normative, this package's own; csrc/cloth.hip follows it operation for operation, DESIGN.md "Hanging garments").  All fp64, every operation
rounded on its own (numpy never contracts to fma; the kernel uses _rn intrinsics), so the device gives the bits of simulate_reference below.

  rest shape   X = (cloth_nocs_verts - 0.5) * rest_scale, rest_scale the longest edge of summary/cloth_canonical_aabb_union
  frame        the gripper frame of the dataset: grip vertex g at the origin, z up, gravity along -z.  Start pose: x = X - X[g], v = 0.  Rest lengths
               are measured in this pose with the expression of `len` below, so a garment at rest has len == l0 to the bit and, without gravity, stays
               where it is
  particles    m_i = density * (sum of the rest areas of the faces at i) / 3, w_i = 1 / m_i; w_g = 0; a vertex of no face (m_i = 0) has w_i = 0
  constraints  distance constraints (i, j, l0, alpha) in ONE list: stretch -- one per unique mesh edge, i < j, sorted lexicographically,
               l0 = |x_i - x_j| in the start pose, alpha_stretch -- then bend -- for every edge of exactly two faces the two opposite vertices
               (k, l), k < l, sorted lexicographically, l0 alike, alpha_bend.  An edge of one face, or of more than two, gets no bend constraint
  colouring    greedy first fit in list order: a constraint takes the smallest colour that no earlier constraint sharing a vertex with it has; the list
               is then grouped by colour with a stable sort.  The colouring fixes the result, so it is part of the definition
  constants    h, inv_h = 1 / h, hg = h * gravity (3), damp = max(0, 1 - h * damping), alpha_t = alpha / (h * h): computed ONCE on the host (step_constants)
               and read by both sides
  substep      for every vertex with w > 0:   v = (v + hg) * damp;  x_prev = x;  p = x + h * v
               for each colour, ascending, for each constraint of it:
                   d = p_i - p_j;  len = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z);  s = (w_i + w_j) + alpha_t
                   len == 0 or s == 0: nothing.  Otherwise dl = -(len - l0) / s;  n = d / len;  p_i += (w_i * dl) * n;  p_j -= (w_j * dl) * n
               for every vertex with w > 0:   v = (p - x_prev) * inv_h;  x = p
               (one projection sweep per substep and the multipliers reset every substep, so none is stored; no two constraints of a colour share a
               vertex, so the order inside a colour cannot matter and a colour is one vectorised numpy statement)

Self-collision (OFF by default: collision_thickness = 0, and then every array, attribute and bit is what it is without this section).  Vertex-vertex
contacts found through contact lists that are rebuilt every few substeps, applied by a Jacobi gather once a substep:

  parameters   collision_thickness t (metres; 0: off), collision_margin (> 0 when on), collision_rebuild R (substeps, >= 1), collision_max_list K
               (in [1, 64]), collision_relax (in (0, 1])
  constants    t2 = t * t, r = t + margin, r2 = r * r: computed ONCE on the host (collision_constants), kept in Garment.collision, read by both sides
  pair         sq(a, b) = (dx*dx + dy*dy) + dz*dz of d = a - b;  rest2_ij = sq(x0_i, x0_j) on the garment's START POSE Garment.x0 (not the state a call
               starts from);  tm2_ij = min(t2, rest2_ij): vertices closer than t at rest are only kept from coming closer than they were, so mesh
               neighbours need no exclusion rule and t may exceed an edge length
  contact list of vertex i at a rebuild, from the positions x at the start of that substep: all j != i with sq(x_i, x_j) <= r2 and tm2_ij > 0, in
               ascending j, cut to the first K; an entry is (j, tm2_ij); the entries cut off are counted as overflow.  Every vertex has a list, those
               with w = 0 too (they are read only as partners).  Rebuilds happen at the substeps s of a call with s % R == 0, s counted from the call's
               first substep: a run split into calls equals one call only when every call but the last is a multiple of R long.  The list is DEFINED
               by brute force over all pairs (contact_lists_reference); a search structure must return exactly this set
  contact pass once a substep, after the last colour and before the velocity pass, on the positions p as the sweep left them.  For every i with
               w_i > 0:  corr = (0, 0, 0);  for each entry in list order:  d = p_i - p_j;  d2 = sq;  active iff d2 < tm2 and d2 > 0 (both strict);
               active:  len = sqrt(d2);  tmin = sqrt(tm2);  s = w_i + w_j;  dl = (tmin - len) / s;  n = d / len;  corr += (w_i * dl) * n (per
               component).  When all vertices have read:  p_i = p_i + relax * corr.  One writer per position, no atomics, an order fixed by the list.
               A garment at rest has no active entry (d2 == rest2 >= tm2), so without gravity nothing moves, to the bit
  diagnostics  per garment and call: contact_overflow (the sum of overflow over the rebuilds), contact_max_list (the longest uncut list),
               contact_travel (the largest, over rebuild intervals and vertices, of sqrt(sq(x_i, x_i at the last rebuild)) / (margin / 2), taken at every
               rebuild after the first and at the end of the call: above 1 a contact may have been missed), contact_active (active entries summed over
               the substeps)

Vertex-face contacts (OFF by default: face_thickness = 0, and then every array, attribute, diagnostic and bit is what it is without this section).  A
vertex is kept off the faces it is no corner of, through face-contact lists built where the vertex lists are built and applied in the same Jacobi gather:

  parameters   face_thickness t_f (metres; 0: off; not negative; positive only with collision_thickness > 0), face_max_list K_f (a whole number in
               [1, 32], FACE_MAX_LIST_CAP); collision_margin, collision_rebuild and collision_relax are shared with the vertex contacts
  constants    tf2 = t_f * t_f, rf = t_f + margin, rf2 = rf * rf, Kf: computed ONCE on the host (face_collision_constants), kept in
               Garment.face_collision, read by both sides
  closest point  point_triangle(q, a, b, c) -> (d2, r, bary): the arithmetic of distance.py's d2, operation for operation (e0, e1, e2, the Gram entries,
               the four reciprocals-or-zero, the clamped segment distances s0, s1, s2, the plane projection (s, t, plane, inside)), which in addition
               names the winner: inside and plane <= min(s0, s1, s2): the plane, r = (w - s*e0) - t*e1, bary = ((1 - s) - t, s, t); otherwise the
               first of s0, s1, s2 equal to the minimum, r the residual that segment squares, u its clamped parameter, bary = (1-u, u, 0) on v0->v1,
               (1-u, 0, u) on v0->v2, (0, 1-u, u) on v1->v2.  d2 is the winner's value: the d2 of distance.point_mesh_sqdist_reference, to the bit
  face list    of vertex i at a rebuild, from the positions x at the start of that substep: every face f with i no corner of f (by index: the squared
               distance of a corner to its own face can be a tiny positive number, l2 * (1 / l2) may be below 1), d2(x_i, tri_f(x)) <= rf2 and
               tm2_if = min(tf2, d2(x0_i, tri_f(x0))) > 0, in ascending f, cut to the first K_f; an entry is (f, tm2_if); the entries cut off are
               counted as overflow.  DEFINED by brute force over all (vertex, face) pairs (face_contact_lists_reference).  Rebuilds at the substeps of
               the vertex lists, s % R == 0.  The travel diagnostic covers these lists too: if no vertex moves more than margin / 2, no
               point-triangle distance changes by more than margin
  contact pass the gather of the vertex pass and its corr.  For i with w_i > 0 the vertex entries come first, in list order (unchanged), then the
               face entries in list order, both on the positions p as the sweep left them.  Entry (f, tm2), (a, b, c) = faces[f]:
               d2, r, bary = point_triangle(p_i, p_a, p_b, p_c);  active iff d2 < tm2 and d2 > 0 (both strict);  active:  len = sqrt(d2);
               tmin = sqrt(tm2);  n = r / len;  s = (w_i + ((b0*b0)*w_a + (b1*b1)*w_b)) + (b2*b2)*w_c;  dl = (tmin - len) / s;
               corr += (w_i * dl) * n.  Then the single p_i = p_i + relax * corr.  The vertex takes its mass-weighted share; THE FACE'S CORNERS DO NOT
               RECEIVE THE REACTION (one writer per position, no atomics: a reaction needs reverse lists with a fixed order, the step after this
               one), so this pass does not conserve momentum and a light face in front of a heavy vertex resolves slowly.  A garment at rest has no
               active entry (d2 == rest d2 >= tm2): without gravity nothing moves, to the bit
  diagnostics  face_contact_overflow, face_contact_max_list, face_contact_active (FACE_CONTACT_STATS): the meaning of their vertex namesakes; they
               join the stats dict only when face contacts are on

NOT modelled: edge-edge contacts, the reaction of a vertex-face contact on the face, continuous collision detection, friction, collision with anything
else, aerodynamic forces, strain limiting, dihedral bending, a random start orientation, moving grippers.  With contacts off the result is a hanging
garment that may pass through itself; with the vertex contacts on, its vertices keep their distance but a vertex can still pass through the middle
of a face larger than the thickness; with the face contacts on as well a vertex is kept off the faces, while two edges can still cross.
"""
import dataclasses
import hashlib

import numpy as np

# "a look", chosen from runs of simulate_reference (DESIGN.md "Hanging garments"); no test depends on them
DEFAULT_GRAVITY = 9.81                 # m / s^2 along -z
DEFAULT_H = 1.0 / 2400.0               # seconds per substep
DEFAULT_DURATION = 3.0                 # seconds simulated
DEFAULT_DAMPING = 4.0                  # 1 / s: v *= 1 - h * damping every substep
DEFAULT_ALPHA_STRETCH = 0.0            # m / N: as stiff as the substep count makes it
DEFAULT_ALPHA_BEND = 0.1               # m / N
DEFAULT_DENSITY = 0.2                  # kg / m^2
# self-collision, used by `simulate --self_collision` only (ClothParams has contacts off by default)
DEFAULT_COLLISION_THICKNESS_FACTOR = 1.5     # thickness = factor * the mean stretch rest length of the garment (mean_stretch_rest_length)
DEFAULT_COLLISION_MARGIN_FACTOR = 1.0        # margin = factor * thickness
DEFAULT_COLLISION_REBUILD = 4                # substeps between two list builds
DEFAULT_COLLISION_MAX_LIST = 64
DEFAULT_COLLISION_RELAX = 1.0
COLLISION_MAX_LIST_CAP = 64                  # CL_MAX_LIST of csrc/cloth.hip
COLLISION_FIELDS = ("collision_thickness", "collision_margin", "collision_rebuild", "collision_max_list", "collision_relax")
# vertex-face contacts, used by `simulate --face_contacts` only
DEFAULT_FACE_THICKNESS_FACTOR = 0.5          # face thickness = factor * the mean stretch rest length of the garment
DEFAULT_FACE_MAX_LIST = 32
FACE_MAX_LIST_CAP = 32                       # CL_FACE_MAX_LIST of csrc/cloth.hip
FACE_COLLISION_FIELDS = ("face_thickness", "face_max_list")


@dataclasses.dataclass(frozen=True)
class ClothParams:
    gravity: float = DEFAULT_GRAVITY
    h: float = DEFAULT_H
    damping: float = DEFAULT_DAMPING
    alpha_stretch: float = DEFAULT_ALPHA_STRETCH
    alpha_bend: float = DEFAULT_ALPHA_BEND
    density: float = DEFAULT_DENSITY
    collision_thickness: float = 0.0       # metres; 0: no contacts
    collision_margin: float = 0.0          # metres; > 0 when contacts are on
    collision_rebuild: int = 1             # substeps between two list builds
    collision_max_list: int = DEFAULT_COLLISION_MAX_LIST
    collision_relax: float = DEFAULT_COLLISION_RELAX
    face_thickness: float = 0.0            # metres; 0: no vertex-face contacts
    face_max_list: int = DEFAULT_FACE_MAX_LIST

    def __post_init__(self):
        vals = dataclasses.asdict(self)
        if not all(np.isfinite(v) for v in vals.values()):
            raise ValueError(f"cloth parameters must be finite, got {vals}")
        if not self.h > 0 or not self.density > 0 or self.damping < 0 or self.alpha_stretch < 0 or self.alpha_bend < 0:
            raise ValueError(f"cloth parameters: h and density must be positive, damping and the compliances not negative, got {vals}")
        if self.collision_thickness < 0 or self.collision_margin < 0:
            raise ValueError(f"cloth parameters: collision_thickness and collision_margin must not be negative, got {vals}")
        if self.collision_thickness > 0 and not self.collision_margin > 0:
            raise ValueError(f"cloth parameters: collision_margin must be positive when collision_thickness is, got {vals}")
        if int(self.collision_rebuild) != self.collision_rebuild or self.collision_rebuild < 1:
            raise ValueError(f"cloth parameters: collision_rebuild must be a whole number >= 1, got {self.collision_rebuild}")
        if int(self.collision_max_list) != self.collision_max_list or not 1 <= self.collision_max_list <= COLLISION_MAX_LIST_CAP:
            raise ValueError(f"cloth parameters: collision_max_list must be a whole number in [1, {COLLISION_MAX_LIST_CAP}], got {self.collision_max_list}")
        if not 0 < self.collision_relax <= 1:
            raise ValueError(f"cloth parameters: collision_relax must lie in (0, 1], got {self.collision_relax}")
        if self.face_thickness < 0:
            raise ValueError(f"cloth parameters: face_thickness must not be negative, got {self.face_thickness}")
        if self.face_thickness > 0 and not self.collision_thickness > 0:
            raise ValueError(f"cloth parameters: face_thickness > 0 needs collision_thickness > 0 (the face contacts share the vertex contacts' margin, "
                             f"rebuild and relax), got {vals}")
        if int(self.face_max_list) != self.face_max_list or not 1 <= self.face_max_list <= FACE_MAX_LIST_CAP:
            raise ValueError(f"cloth parameters: face_max_list must be a whole number in [1, {FACE_MAX_LIST_CAP}], got {self.face_max_list}")

    @property
    def contacts(self):
        return self.collision_thickness > 0

    @property
    def face_contacts(self):
        return self.face_thickness > 0


def step_constants(params):
    """the per-step numbers both sides read -> dict of python floats (fp64): h, inv_h, hg (3), damp, alpha_t_stretch, alpha_t_bend"""
    h = np.float64(params.h)
    g = np.array([0.0, 0.0, -float(params.gravity)], dtype=np.float64)
    return {"h": float(h), "inv_h": float(np.float64(1.0) / h), "hg": [float(c) for c in h * g],
            "damp": float(max(np.float64(0.0), np.float64(1.0) - h * np.float64(params.damping))),
            "alpha_t_stretch": float(np.float64(params.alpha_stretch) / (h * h)), "alpha_t_bend": float(np.float64(params.alpha_bend) / (h * h))}


def collision_constants(params):
    """the contact numbers both sides read -> None with contacts off, else a dict: t2, r, r2, half_margin, relax (python floats, fp64), K, R (ints)"""
    if not params.contacts:
        return None
    t, m = np.float64(params.collision_thickness), np.float64(params.collision_margin)
    r = t + m
    return {"t2": float(t * t), "r": float(r), "r2": float(r * r), "half_margin": float(m / np.float64(2.0)), "relax": float(params.collision_relax),
            "K": int(params.collision_max_list), "R": int(params.collision_rebuild)}


def face_collision_constants(params):
    """the face-contact numbers both sides read -> None with face contacts off, else a dict: tf2, rf, rf2 (python floats, fp64), Kf (int)"""
    if not params.face_contacts:
        return None
    t, m = np.float64(params.face_thickness), np.float64(params.collision_margin)
    rf = t + m
    return {"tf2": float(t * t), "rf": float(rf), "rf2": float(rf * rf), "Kf": int(params.face_max_list)}


def substeps_of(duration, h):
    return int(round(float(duration) / float(h)))


# ------------------------------------------------------------------------------------------------ topology
def _faces(faces):
    faces = np.asarray(faces)
    if faces.size == 0:
        return np.zeros((0, 3), dtype=np.int64)
    if faces.dtype.kind not in "iu":
        raise TypeError(f"faces: expected an integer array, got {faces.dtype}")
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces: expected an (F, 3) array, got {faces.shape}")
    return faces.astype(np.int64)


def constraint_pairs(faces):
    """-> (stretch (Ns, 2), bend (Nb, 2)) int64 in the list order of the definition.  Reads no vertex, so an index outside the mesh passes through."""
    faces = _faces(faces)
    corners = np.stack([faces[:, [0, 1, 2]], faces[:, [1, 2, 0]], faces[:, [2, 0, 1]]], axis=1).reshape(-1, 3)     # (edge a, edge b, opposite)
    corners = corners[corners[:, 0] != corners[:, 1]]                                     # a face that names a vertex twice has no edge there
    if len(corners) == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64)
    edges = np.sort(corners[:, :2], axis=1)
    stretch, inverse, count = np.unique(edges, axis=0, return_inverse=True, return_counts=True)       # rows sorted lexicographically
    inverse = inverse.reshape(-1)
    order = np.argsort(inverse, kind="stable")
    first = np.concatenate([[0], np.cumsum(count)[:-1]])[count == 2]
    opp = np.sort(np.stack([corners[order[first], 2], corners[order[first + 1], 2]], axis=1), axis=1)
    opp = opp[opp[:, 0] != opp[:, 1]]                                                     # the same face twice: no pair
    bend = opp[np.lexsort((opp[:, 1], opp[:, 0]))] if len(opp) else np.zeros((0, 2), np.int64)
    return stretch.astype(np.int64), bend.astype(np.int64)


def first_fit_colours(pairs):
    """greedy first fit in list order -> (C,) int64"""
    used = {}
    out = np.zeros(len(pairs), dtype=np.int64)
    for c, (i, j) in enumerate(pairs.tolist()):
        taken = used.get(i, 0) | used.get(j, 0)
        free = ~taken & (taken + 1)                    # the lowest clear bit
        out[c] = free.bit_length() - 1
        used[i] = used.get(i, 0) | free
        used[j] = used.get(j, 0) | free
    return out


@dataclasses.dataclass(frozen=True)
class Topology:
    pairs: np.ndarray            # (C, 2) int64, grouped by colour
    is_bend: np.ndarray          # (C,) bool
    colour_off: np.ndarray       # (K + 1,) int64: colour k owns pairs[colour_off[k] : colour_off[k + 1]]
    n_stretch: int
    n_bend: int


_TOPOLOGY_CACHE = {}
_TOPOLOGY_CACHE_MAX = 64


def topology(faces):
    """the coloured constraint list of a faces array, built once per array (garments of one template share it)"""
    faces = np.ascontiguousarray(_faces(faces))
    key = (faces.shape[0], hashlib.sha1(faces.tobytes()).hexdigest())
    hit = _TOPOLOGY_CACHE.get(key)
    if hit is not None:
        return hit
    stretch, bend = constraint_pairs(faces)
    pairs = np.concatenate([stretch, bend])
    is_bend = np.arange(len(pairs)) >= len(stretch)
    colour = first_fit_colours(pairs)
    order = np.argsort(colour, kind="stable")
    k = int(colour.max()) + 1 if len(colour) else 0
    off = np.concatenate([[0], np.cumsum(np.bincount(colour, minlength=k))]).astype(np.int64)
    topo = Topology(pairs[order], is_bend[order], off, len(stretch), len(bend))
    for a in (topo.pairs, topo.is_bend, topo.colour_off):
        a.setflags(write=False)
    if len(_TOPOLOGY_CACHE) >= _TOPOLOGY_CACHE_MAX:
        _TOPOLOGY_CACHE.pop(next(iter(_TOPOLOGY_CACHE)))
    _TOPOLOGY_CACHE[key] = topo
    return topo


# ------------------------------------------------------------------------------------------------ a garment
def _norm3(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def rest_scale_of(canonical_aabb):
    """the longest edge of summary/cloth_canonical_aabb_union"""
    box = np.asarray(canonical_aabb, dtype=np.float64)
    return float((box[1] - box[0]).max())


def rest_shape(nocs_verts, rest_scale):
    return (np.asarray(nocs_verts, dtype=np.float64) - 0.5) * np.float64(rest_scale)


@dataclasses.dataclass
class Garment:
    """what one garment's simulation reads: everything fp64 / int64 numpy"""
    x0: np.ndarray               # (V, 3) start pose: the rest shape with the grip vertex at the origin
    w: np.ndarray                # (V,) inverse masses
    pairs: np.ndarray            # (C, 2), grouped by colour
    is_bend: np.ndarray          # (C,) bool
    l0: np.ndarray               # (C,)
    alpha_t: np.ndarray          # (C,)
    colour_off: np.ndarray       # (K + 1,)
    consts: dict                 # step_constants
    grip: int
    n_massless: int              # vertices of no face (the grip vertex is not counted)
    n_stretch: int
    n_bend: int
    bad_index: bool              # a face names a vertex outside [0, V): only a garment built with check=False carries one
    collision: dict = None       # collision_constants: None with contacts off
    faces: np.ndarray = None     # (F, 3) int64, the mesh's faces in their order (garment() always fills it)
    face_collision: dict = None  # face_collision_constants: None with face contacts off


def garment(X, faces, grip, params, check=True):
    """the Garment of a rest shape X (V, 3), its faces and the grip vertex.  check=False lets a face index outside [0, V) through (its rest lengths and
    areas are then read at a clipped index and mean nothing): the device entry flags such an index itself and never dereferences it."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError(f"verts: expected a (V, 3) array, got {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError("cloth: a rest-shape vertex is not finite")
    V = len(X)
    grip = int(grip)
    if not 0 <= grip < V:
        raise ValueError(f"cloth: grip vertex {grip} outside [0, {V})")
    faces = _faces(faces)
    bad = bool(len(faces) and (faces.min() < 0 or faces.max() >= V))
    if bad and check:
        raise IndexError("cloth: a face index is out of bounds for its mesh's vertices")
    topo = topology(faces)
    safe = np.clip(faces, 0, V - 1)
    a, b, c = X[safe[:, 0]], X[safe[:, 1]], X[safe[:, 2]]
    area = 0.5 * _norm3(np.cross(b - a, c - a))
    mass = np.zeros(V, dtype=np.float64)
    for k in range(3):
        np.add.at(mass, safe[:, k], area)              # unbuffered: face order, one addition after the other
    mass = np.float64(params.density) * mass / 3.0
    w = np.zeros(V, dtype=np.float64)
    np.divide(1.0, mass, out=w, where=mass > 0)
    n_massless = int((mass == 0).sum()) - int(mass[grip] == 0)
    w[grip] = 0.0
    if not np.isfinite(w).all():
        raise ValueError("cloth: an inverse mass is not finite (a face of vanishing area)")
    consts = step_constants(params)
    x0 = X - X[grip]
    ij = np.clip(topo.pairs, 0, V - 1)
    l0 = _norm3(x0[ij[:, 0]] - x0[ij[:, 1]]) if len(ij) else np.zeros(0)      # measured in the start pose, as the sweep measures len
    alpha_t = np.where(topo.is_bend, consts["alpha_t_bend"], consts["alpha_t_stretch"]).astype(np.float64)
    return Garment(x0, w, topo.pairs, topo.is_bend, l0, alpha_t, topo.colour_off, consts, grip, n_massless, topo.n_stretch, topo.n_bend, bad,
                   collision_constants(params), faces, face_collision_constants(params))


def garment_from_nocs(nocs_verts, faces, grip, rest_scale, params, check=True):
    return garment(rest_shape(nocs_verts, rest_scale), faces, grip, params, check=check)


def state_arrays(g, x, v, who="cloth"):
    """(x, v) float64 (V, 3) copies of a state (None: the start pose / rest), refused when not finite"""
    x = np.array(g.x0 if x is None else x, dtype=np.float64)
    v = np.zeros_like(g.x0) if v is None else np.array(v, dtype=np.float64)
    if x.shape != g.x0.shape or v.shape != g.x0.shape:
        raise ValueError(f"{who}: x and v must be {g.x0.shape}, got {x.shape} and {v.shape}")
    if not (np.isfinite(x).all() and np.isfinite(v).all()):
        raise ValueError(f"{who}: a position or velocity is not finite")
    return x, v


# ------------------------------------------------------------------------------------------------ the restatement
def project_colour(p, w, i, j, l0, alpha_t):
    """one colour of the sweep, in place on p: the constraints (i, j, l0, alpha_t) share no vertex"""
    pi, pj = p[i], p[j]
    d = pi - pj
    length = _norm3(d)
    wi, wj = w[i], w[j]
    s = (wi + wj) + alpha_t
    act = (length != 0) & (s != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dl = -(length - l0) / s
        n = d / length[:, None]
        new_i = pi + (wi * dl)[:, None] * n
        new_j = pj - (wj * dl)[:, None] * n
    p[i[act]] = new_i[act]
    p[j[act]] = new_j[act]


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def contact_lists_reference(g, x, chunk=256):
    """the contact lists of the definition for the positions x, by brute force over all pairs (`chunk` rows at a time, so V x V is never held at once)
    -> ((idx (V, K) int32, tm2 (V, K) float64), counts (V,) int64, overflow (V,) int64): row i holds its first counts[i] entries in ascending j, the
    rest of the row is (-1, 0); overflow[i] entries were cut off, so counts + overflow is the uncut length"""
    c = g.collision
    if c is None:
        raise ValueError("contact_lists_reference: the garment has contacts off (collision_thickness = 0)")
    x = np.asarray(x, dtype=np.float64)
    if x.shape != g.x0.shape:
        raise ValueError(f"contact_lists_reference: x must be {g.x0.shape}, got {x.shape}")
    V, K = len(x), c["K"]
    t2, r2 = np.float64(c["t2"]), np.float64(c["r2"])
    idx = np.full((V, K), -1, dtype=np.int32)
    tm2 = np.zeros((V, K), dtype=np.float64)
    counts = np.zeros(V, dtype=np.int64)
    overflow = np.zeros(V, dtype=np.int64)
    cols = np.arange(V)
    for a in range(0, V, int(chunk)):
        rows = np.arange(a, min(a + int(chunk), V))
        rest2 = _sq3(g.x0[rows, None, :] - g.x0[None, :, :])
        near = (_sq3(x[rows, None, :] - x[None, :, :]) <= r2) & (np.minimum(t2, rest2) > 0) & (rows[:, None] != cols[None, :])
        rank = np.cumsum(near, axis=1) - 1                    # the place of j among the row's partners, ascending j
        total = near.sum(axis=1)
        n, j = np.nonzero(near & (rank < K))
        idx[rows[n], rank[n, j]] = j
        tm2[rows[n], rank[n, j]] = np.minimum(t2, rest2[n, j])
        counts[rows] = np.minimum(total, K)
        overflow[rows] = total - counts[rows]
    return (idx, tm2), counts, overflow


def contact_entries(g, lists, counts):
    """the list entries the contact pass reads, flat and in its order (vertex by vertex, list order inside a vertex), of the vertices with w > 0
    -> (i, j, tm2)"""
    idx, tm2 = lists
    keep = (np.arange(idx.shape[1])[None, :] < np.asarray(counts)[:, None]) & (g.w > 0)[:, None]
    i, k = np.nonzero(keep)                                   # row-major: the order of the definition
    return i, idx[i, k].astype(np.int64), tm2[i, k]


def contact_pass(p, w, entries, relax, face=None):
    """the contact pass of the definition, in place on p -> (active vertex entries, active face entries); face: None (no face entries: the second
    count is 0) or (faces (F, 3), face_contact_entries): the face entries follow the vertex entries in the same corr"""
    i, j, tm2 = entries
    d = p[i] - p[j]
    d2 = _sq3(d)
    act = (d2 < tm2) & (d2 > 0)
    i, j, d, d2, tm2 = i[act], j[act], d[act], d2[act], tm2[act]
    length = np.sqrt(d2)
    wi = w[i]
    dl = (np.sqrt(tm2) - length) / (wi + w[j])
    n = d / length[:, None]
    corr = np.zeros_like(p)
    np.add.at(corr, i, (wi * dl)[:, None] * n)                # unbuffered: entry after entry, so list order inside a vertex
    face_active = 0 if face is None else face_contact_gather(corr, p, w, face[0], face[1])
    live = w > 0
    p[live] = p[live] + np.float64(relax) * corr[live]
    return int(act.sum()), face_active


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _rcp_or_zero(x):
    return np.where(x > 0.0, 1.0 / np.where(x > 0.0, x, 1.0), 0.0)


def _seg_closest(w, e, wd, inv):
    """distance.py's _seg, which also returns what it squares: (r.r, r (3 components), the clamped parameter)"""
    u = np.fmin(np.fmax(wd * inv, 0.0), 1.0)
    r = [w[k] - u * e[k] for k in range(3)]
    return _dot3(r, r), r, u


def point_triangle(q, a, b, c):
    """the closest point of the triangle (a, b, c) to q, all (..., 3) and broadcast against each other -> (d2 (...), r (..., 3), bary (..., 3)): d2 the
    squared distance of distance.point_mesh_sqdist_reference to the bit, r = q - the closest point as the winner of the definition computes it, bary
    the closest point's weights on (a, b, c)"""
    q, a, b, c = np.broadcast_arrays(*(np.asarray(p, dtype=np.float64) for p in (q, a, b, c)))
    q, v0, v1, v2 = ([p[..., k] for k in range(3)] for p in (q, a, b, c))
    with np.errstate(all="ignore"):
        e0, e1, e2 = ([i[k] - j[k] for k in range(3)] for i, j in ((v1, v0), (v2, v0), (v2, v1)))
        ga, gb, gc, l2 = _dot3(e0, e0), _dot3(e0, e1), _dot3(e1, e1), _dot3(e2, e2)
        idet, ia, ic, ie2 = _rcp_or_zero(ga * gc - gb * gb), _rcp_or_zero(ga), _rcp_or_zero(gc), _rcp_or_zero(l2)
        w = [q[k] - v0[k] for k in range(3)]
        d0, d1 = _dot3(w, e0), _dot3(w, e1)
        s0, r0, u0 = _seg_closest(w, e0, d0, ia)
        s1, r1, u1 = _seg_closest(w, e1, d1, ic)
        u = [q[k] - v1[k] for k in range(3)]
        s2, r2, u2 = _seg_closest(u, e2, _dot3(u, e2), ie2)
        s, t = (gc * d0 - gb * d1) * idet, (ga * d1 - gb * d0) * idet
        rp = [(w[k] - s * e0[k]) - t * e1[k] for k in range(3)]
        plane = _dot3(rp, rp)
        inside = (idet > 0.0) & (s >= 0.0) & (t >= 0.0) & (s + t <= 1.0)
        seg = np.fmin(np.fmin(s0, s1), s2)
        win_p = inside & (plane <= seg)
        win_0 = ~win_p & (s0 == seg)
        win_1 = ~win_p & ~win_0 & (s1 == seg)
        one, zero = np.ones_like(seg), np.zeros_like(seg)
        d2 = np.where(win_p, plane, seg)
        r = np.stack([np.where(win_p, rp[k], np.where(win_0, r0[k], np.where(win_1, r1[k], r2[k]))) for k in range(3)], axis=-1)
        b0 = np.where(win_p, (one - s) - t, np.where(win_0, one - u0, np.where(win_1, one - u1, zero)))
        b1 = np.where(win_p, s, np.where(win_0, u0, np.where(win_1, zero, one - u2)))
        b2 = np.where(win_p, t, np.where(win_0, zero, np.where(win_1, u1, u2)))
    return d2, r, np.stack([b0, b1, b2], axis=-1)


def _face_corners(g):
    if g.faces is None:
        raise ValueError("cloth face contacts: the garment carries no faces (build it with cloth.garment)")
    return np.asarray(g.faces, dtype=np.int64).reshape(-1, 3)


def face_contact_lists_reference(g, x, chunk=256):
    """the face-contact lists of the definition for the positions x, by brute force over all (vertex, face) pairs (`chunk` vertices at a time)
    -> ((idx (V, Kf) int32, tm2 (V, Kf) float64), counts (V,) int64, overflow (V,) int64): row i holds its first counts[i] entries in ascending f,
    the rest of the row is (-1, 0); overflow[i] entries were cut off"""
    c = g.face_collision
    if c is None:
        raise ValueError("face_contact_lists_reference: the garment has face contacts off (face_thickness = 0)")
    if g.bad_index:
        raise IndexError("cloth: a face index is out of bounds for its mesh's vertices")
    x = np.asarray(x, dtype=np.float64)
    if x.shape != g.x0.shape:
        raise ValueError(f"face_contact_lists_reference: x must be {g.x0.shape}, got {x.shape}")
    faces = _face_corners(g)
    V, F, K = len(x), len(faces), c["Kf"]
    tf2, rf2 = np.float64(c["tf2"]), np.float64(c["rf2"])
    idx = np.full((V, K), -1, dtype=np.int32)
    tm2 = np.zeros((V, K), dtype=np.float64)
    counts = np.zeros(V, dtype=np.int64)
    overflow = np.zeros(V, dtype=np.int64)
    if F == 0:
        return (idx, tm2), counts, overflow
    fa, fb, fc = faces[:, 0], faces[:, 1], faces[:, 2]
    for a in range(0, V, int(chunk)):
        rows = np.arange(a, min(a + int(chunk), V))
        now = point_triangle(x[rows, None, :], x[None, fa, :], x[None, fb, :], x[None, fc, :])[0]
        rest = np.minimum(tf2, point_triangle(g.x0[rows, None, :], g.x0[None, fa, :], g.x0[None, fb, :], g.x0[None, fc, :])[0])
        corner = (rows[:, None] == fa[None, :]) | (rows[:, None] == fb[None, :]) | (rows[:, None] == fc[None, :])
        near = (now <= rf2) & (rest > 0) & ~corner
        rank = np.cumsum(near, axis=1) - 1
        total = near.sum(axis=1)
        n, f = np.nonzero(near & (rank < K))
        idx[rows[n], rank[n, f]] = f
        tm2[rows[n], rank[n, f]] = rest[n, f]
        counts[rows] = np.minimum(total, K)
        overflow[rows] = total - counts[rows]
    return (idx, tm2), counts, overflow


def face_contact_entries(g, lists, counts):
    """the face-list entries the contact pass reads, flat and in its order, of the vertices with w > 0 -> (i, f, tm2)"""
    return contact_entries(g, lists, counts)


def face_contact_gather(corr, p, w, faces, entries):
    """the face entries (i, f, tm2) of the contact pass, added to corr in place entry after entry (after the vertex entries: corr carries their sum)
    -> the number of active entries; p is read only"""
    i, f, tm2 = entries
    if len(i) == 0:
        return 0
    ca, cb, cc = faces[f, 0], faces[f, 1], faces[f, 2]
    d2, r, bary = point_triangle(p[i], p[ca], p[cb], p[cc])
    act = (d2 < tm2) & (d2 > 0)
    i, d2, r, bary, tm2, ca, cb, cc = i[act], d2[act], r[act], bary[act], tm2[act], ca[act], cb[act], cc[act]
    length = np.sqrt(d2)
    wi = w[i]
    b0, b1, b2 = bary[:, 0], bary[:, 1], bary[:, 2]
    s = (wi + ((b0 * b0) * w[ca] + (b1 * b1) * w[cb])) + (b2 * b2) * w[cc]
    dl = (np.sqrt(tm2) - length) / s
    n = r / length[:, None]
    np.add.at(corr, i, (wi * dl)[:, None] * n)                # unbuffered: entry after entry, so list order inside a vertex
    return int(act.sum())


def contact_travel(g, x, x_ref):
    """sqrt(the largest sq(x_i, x_ref_i)) / (margin / 2): sqrt and the division are monotone, so this is the largest of the definition's quotients"""
    if len(x) == 0:
        return 0.0
    return float(np.sqrt(_sq3(x - x_ref).max()) / np.float64(g.collision["half_margin"]))


def substep(g, x, v, entries=None, face_entries=None):
    """one substep of the definition, in place on x and v -> (active vertex entries, active face entries); entries: contact_entries of the current
    lists (None: no contact pass); face_entries: face_contact_entries of the current face lists (None: no face entries; they need `entries`)"""
    c = g.consts
    h, inv_h, damp, hg = np.float64(c["h"]), np.float64(c["inv_h"]), np.float64(c["damp"]), np.array(c["hg"], dtype=np.float64)
    live = g.w > 0
    v[live] = (v[live] + hg) * damp
    x_prev = x.copy()
    p = x.copy()
    p[live] = x[live] + h * v[live]
    off = g.colour_off
    for k in range(len(off) - 1):
        sl = slice(off[k], off[k + 1])
        project_colour(p, g.w, g.pairs[sl, 0], g.pairs[sl, 1], g.l0[sl], g.alpha_t[sl])
    active = (0, 0)
    if entries is not None:
        face = None if face_entries is None else (_face_corners(g), face_entries)
        active = contact_pass(p, g.w, entries, g.collision["relax"], face=face)
    v[live] = (p[live] - x_prev[live]) * inv_h
    x[live] = p[live]
    return active


CONTACT_STATS = ("contact_overflow", "contact_max_list", "contact_travel", "contact_active")
FACE_CONTACT_STATS = ("face_contact_overflow", "face_contact_max_list", "face_contact_active")


def simulate_reference(g, substeps, x=None, v=None, stats=False, observe=None):
    """`substeps` substeps from (x, v) (None: the start pose at rest) -> (x, v) float64 (V, 3), new arrays; stats=True: (x, v, the contact diagnostics
    of the definition as a dict, all 0 with contacts off; with face contacts on FACE_CONTACT_STATS join it).  With contacts on the lists are rebuilt at
    the substeps s with s % R == 0.  observe: called as observe(s, x, v) after every substep s (the arrays are the run's own: read, do not write)."""
    if g.bad_index:
        raise IndexError("cloth: a face index is out of bounds for its mesh's vertices")
    x, v = state_arrays(g, x, v, "simulate_reference")
    out = {"contact_overflow": 0, "contact_max_list": 0, "contact_travel": 0.0, "contact_active": 0}
    if g.face_collision is not None and g.collision is None:
        raise ValueError("simulate_reference: face contacts need the vertex contacts on (collision_thickness > 0)")
    if g.collision is None:
        for s in range(int(substeps)):
            substep(g, x, v)
            if observe is not None:
                observe(s, x, v)
        return (x, v, out) if stats else (x, v)
    entries = face_entries = x_ref = None
    faces_on = g.face_collision is not None
    if faces_on:
        out.update({k: 0 for k in FACE_CONTACT_STATS})
    for s in range(int(substeps)):
        if s % g.collision["R"] == 0:
            if x_ref is not None:
                out["contact_travel"] = max(out["contact_travel"], contact_travel(g, x, x_ref))
            lists, counts, overflow = contact_lists_reference(g, x)
            out["contact_overflow"] += int(overflow.sum())
            out["contact_max_list"] = max(out["contact_max_list"], int((counts + overflow).max(initial=0)))
            entries, x_ref = contact_entries(g, lists, counts), x.copy()
            if faces_on:
                lists, counts, overflow = face_contact_lists_reference(g, x)
                out["face_contact_overflow"] += int(overflow.sum())
                out["face_contact_max_list"] = max(out["face_contact_max_list"], int((counts + overflow).max(initial=0)))
                face_entries = face_contact_entries(g, lists, counts)
        active, face_active = substep(g, x, v, entries, face_entries)
        out["contact_active"] += active
        if faces_on:
            out["face_contact_active"] += face_active
        if observe is not None:
            observe(s, x, v)
    if x_ref is not None:
        out["contact_travel"] = max(out["contact_travel"], contact_travel(g, x, x_ref))
    return (x, v, out) if stats else (x, v)


def mean_stretch_rest_length(g):
    """the mean rest length of the stretch constraints: (sum of l0 over them) / their number, 0 for a garment without one"""
    stretch = ~g.is_bend
    return float(g.l0[stretch].sum() / stretch.sum()) if stretch.any() else 0.0


# ------------------------------------------------------------------------------------------------ diagnostics
def diagnostics(g, x, v):
    """-> {"kinetic_energy": sum m |v|^2 / 2 over the moving vertices, "max_stretch_strain": max |len / l0 - 1| over the stretch constraints,
    "massless_vertices": count}"""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    live = g.w > 0
    ke = float(0.5 * ((v[live] ** 2).sum(axis=1) / g.w[live]).sum())
    stretch = ~g.is_bend & (g.l0 > 0)
    strain = 0.0
    if stretch.any():
        i, j = g.pairs[stretch, 0], g.pairs[stretch, 1]
        strain = float(np.abs(_norm3(x[i] - x[j]) / g.l0[stretch] - 1.0).max())
    return {"kinetic_energy": ke, "max_stretch_strain": strain, "massless_vertices": int(g.n_massless)}
