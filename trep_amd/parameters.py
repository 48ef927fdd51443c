"""Per-trajectory parameter tables: validation and packing against a ``System`` (host only, no GPU).

A batch can run every trajectory with its own masses / inertias, gravity and damping (include/trep_amd.h,
tg_batch_set_parameters).  A table has ``rows`` rows; trajectory t uses row t // group.  Its three blocks:

=========  ==================  ===============================================================================
name       shape per row       meaning
=========  ==================  ===============================================================================
inertia    [n_bodies][4]       (mass, Ixx, Iyy, Izz) of every massive frame in ``system.masses`` order
                               (the arguments of ``Frame.set_mass``)
gravity    [3]                 the gravity vector: the sum over the system's ``Gravity`` potentials
damping    [nd]                total damping coefficient of every dynamic config in ``system.dyn_configs`` order
                               (the sum of ``Damping.coefficient_array()``)
=========  ==================  ===============================================================================

Any block may be omitted (``None``): every row then has the system's own values (all three omitted: one row of them).  A block may be one row (shape per
row, or a leading axis of 1) and is then broadcast to all rows.  A row acts as the system rebuilt with its values; a
frame massless in the system stays massless, since only the massive frames have an inertia entry.
"""
import numpy as np

from .dynamics import Damping, Gravity

NAMES = ("inertia", "gravity", "damping")


def base_values(system):
    """The system's own values as a dict of arrays: inertia [n_bodies][4], gravity [3] (None without a Gravity potential),
    damping [nd] (None without a Damping force)."""
    inertia = np.array([[f._mass, f._Ixx, f._Iyy, f._Izz] for f in system.masses], dtype=np.float64).reshape(-1, 4)
    gravities = [p for p in system.potentials if isinstance(p, Gravity)]
    dampings = [f for f in system.forces if isinstance(f, Damping)]
    gravity = np.sum([np.array(p._gravity, dtype=np.float64) for p in gravities], axis=0) if gravities else None
    damping = np.sum([f.coefficient_array() for f in dampings], axis=0) if dampings else None
    if damping is not None:
        damping = np.asarray(damping, dtype=np.float64).reshape(len(system.dyn_configs))
    return {"inertia": inertia, "gravity": gravity, "damping": damping}


def _block(name, value, row_shape):
    a = np.asarray(value, dtype=np.float64)
    if a.shape == row_shape:
        a = a[None]
    if a.ndim != len(row_shape) + 1 or a.shape[1:] != row_shape:
        raise ValueError("%s: expected shape [rows]%s, got %s" % (name, list(row_shape), list(np.shape(value))))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s: values must be finite" % name)
    return a.shape[0], a


def pack(system, batch, inertia=None, gravity=None, damping=None, group=1):
    """Validate keyword arrays against `system` and a batch of `batch` trajectories.  Returns (rows, group, blocks), where
    blocks maps each given name to a contiguous float64 array [rows][...] (single rows broadcast) and omitted names to None.
    Raises ValueError for shapes that do not fit, non-finite values, or a gravity / damping block on a system without a
    Gravity potential / Damping force."""
    base = base_values(system)
    n_bodies, nd = base["inertia"].shape[0], len(system.dyn_configs)
    group = int(group)
    if group <= 0:
        raise ValueError("group must be positive, got %d" % group)
    if gravity is not None and base["gravity"] is None:
        raise ValueError("gravity: the system has no Gravity potential")
    if damping is not None and base["damping"] is None:
        raise ValueError("damping: the system has no Damping force")
    given = {}
    shapes = {"inertia": (n_bodies, 4), "gravity": (3,), "damping": (nd,)}
    for name, value in zip(NAMES, (inertia, gravity, damping)):
        if value is not None:
            given[name] = _block(name, value, shapes[name])
    counts = set(n for n, _ in given.values() if n != 1)
    if len(counts) > 1:
        raise ValueError("parameter blocks have different row counts: %s" % sorted(counts))
    rows = counts.pop() if counts else 1      # one row: the whole batch, whatever the group
    if rows != 1 and rows * group != batch:
        raise ValueError("rows * group must equal the batch size: %d * %d != %d" % (rows, group, batch))
    blocks = {}
    for name in NAMES:
        if name in given:
            n, a = given[name]
            blocks[name] = np.ascontiguousarray(np.broadcast_to(a, (rows,) + shapes[name]) if n == 1 else a)
        else:
            blocks[name] = None
    return rows, (group if rows > 1 else 1), blocks


def row_of(trajectory, group):
    """The row trajectory `trajectory` (its batch index) uses."""
    return int(trajectory) // int(group)
