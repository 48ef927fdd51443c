"""Specification of the batched tape measures (BatchMidpointVI.tape_measures, tg_batch_tape_measures): the five arrays of one state
through the host TapeMeasure accessors (reference(): length(), velocity(), length_dq(), velocity_dq(), length_dqdq() of
trep_amd/tapemeasure.py, themselves held to the reference project's recorded values by test_elements.py), a table of seeded states and
measures per system, the comparison with the project's bounds, and the closed formulas of the issue in numpy with the mistakes a kernel
could make (formulas(mutant=...)), so that the tests can show that the table tells them apart.  Test infrastructure only.

A measure is a list of indices into system.frames.  L, V [T]; LQ, VQ [T][nq]; LQQ [T][nq][nq]."""
import collections
import functools

import numpy as np

import common
import frame_kinematics_reference as fr

SYSTEMS = ("extensor_tendon", "puppet40", "scissor4", "spatial_loop", "mixed_loop", "pend_on_cart", "ladder_mixed")
N_STATES = {"puppet40": 3}             # seeded states of a system (default 6): the host Hessian of the six strings takes about 1 s per state
Q_RANGE, DQ_RANGE = 1.5, 2.0
FIELDS = ("length", "velocity", "length_dq", "velocity_dq", "length_dqdq")
# relative to max(1, |want|inf): length and velocity as g / vb of tests/test_frames.py, length_dq as p_dq, the two second-order arrays as that
# file's second-order accessors
TOL = {"length": 1e-12, "velocity": 1e-12, "length_dq": 1e-11, "velocity_dq": 1e-11, "length_dqdq": 1e-11}
MIN_SEGMENT = 0.05                     # every segment of every table state is at least this long
MUTANTS = ("descendant_axis", "prismatic_ancestor_rotary", "diagonal_dropped", "ljlk_dropped", "common_not_excluded", "boundary_off_by_one",
           "closed_line", "state_off_by_one")

Arrays = collections.namedtuple("Arrays", FIELDS)


def _back_and_forth(a, b, segments):
    return [a if i % 2 == 0 else b for i in range(segments + 1)]


@functools.lru_cache(maxsize=None)
def system_of(name):
    return common.build(name)


@functools.lru_cache(maxsize=None)
def measures(name):
    """The measures of a system's table, as tuples of frame indices."""
    system = system_of(name)[0]
    at = lambda n: [f.name for f in system.frames].index(n)
    if name == "extensor_tendon":        # the recorded tape of tests/golden/elements.npz first; a five-frame tendon; one segment
        golden = [at(str(n)) for n in common.golden("elements")["tape_frames"]]
        out = [golden, [at("A"), at("B"), at("C"), at("E"), at("I")], [at("World"), at("I")], golden]
    elif name == "puppet40":             # the six strings: the lengths their Distance constraints fix
        out = [[at(s + "_string_control"), at(s + "_string_hook")] for s in ("upper_torso", "lower_torso", "left_arm", "right_arm", "left_leg", "right_leg")]
    elif name == "scissor4":             # one segment; end points that share ancestors; 17 segments back and forth (two passes); a repeat
        out = [[0, 13], [3, 13], _back_and_forth(13, 25, 17), [6, 0, 25, 12], [3, 13]]
    elif name == "spatial_loop":         # behind the rotated const_se3 and the kinematic rotary config; across the prismatic s; two constants
        out = [[0, 8], [13, 15], [9, 11], [0, 11, 2], [15, 8, 4, 12], [2, 6]]
    elif name == "mixed_loop":           # the kinematic prismatic lift; across the kinematic rotary kr; a constant; shared ancestors; a rotary end
        out = [[0, 9], [3, 6], [18, 16], [4, 8], [20, 8, 15, 12], [14, 15]]
    elif name == "pend_on_cart":         # (Cart and PendulumBase share an origin: never consecutive); 18 segments back and forth
        out = [[0, 3], [1, 3], _back_and_forth(3, 0, 18), [0, 3]]
    elif name == "ladder_mixed":         # tip to tip; a constant; shared ancestors; behind the rotated fixed frame
        out = [[15, 30], [0, 32], [4, 15], [0, 8, 23, 32], [11, 8]]
    return tuple(tuple(int(f) for f in m) for m in out)


def reference(system, q, dq, measure_list):
    """The five arrays of the measures at the state (q, dq), through the host accessors.  Sets system.q / system.dq."""
    from trep_amd import TapeMeasure
    system.q, system.dq = np.asarray(q, dtype=float), np.asarray(dq, dtype=float)
    configs = system.configs
    nq, T = len(configs), len(measure_list)
    out = Arrays(np.zeros(T), np.zeros(T), np.zeros((T, nq)), np.zeros((T, nq)), np.zeros((T, nq, nq)))
    done = {}
    for t, m in enumerate(measure_list):
        m = tuple(m)
        if m in done:
            for a in out:
                a[t] = a[done[m]]
            continue
        done[m] = t
        tape = TapeMeasure(system, [system.frames[f] for f in m])
        out.length[t], out.velocity[t] = tape.length(), tape.velocity()
        for k, c in enumerate(configs):
            out.length_dq[t, k], out.velocity_dq[t, k] = tape.length_dq(c), tape.velocity_dq(c)
            for j, cj in enumerate(configs):
                out.length_dqdq[t, j, k] = tape.length_dqdq(cj, c)
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def states(name):
    """(q [n][nq], dq [n][nq]): the seeded states of a system."""
    d = system_of(name)[1]
    n, nq = N_STATES.get(name, 6), int(d.n_configs)
    rng = np.random.default_rng(common.tb_seed("tape measures", name))
    return rng.uniform(-Q_RANGE, Q_RANGE, (n, nq)), rng.uniform(-DQ_RANGE, DQ_RANGE, (n, nq))


def _stack(rows):
    out = Arrays(*[np.stack([getattr(r, f) for r in rows]) for f in FIELDS])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def state_references(name):
    """reference() of every seeded state over the system's measures, stacked: arrays [n][T]...; computed once, never modified."""
    system = system_of(name)[0]
    q, dq = states(name)
    return _stack([reference(system, q[i], dq[i], measures(name)) for i in range(len(q))])


@functools.lru_cache(maxsize=None)
def state_formulas(name):
    system = system_of(name)[0]
    q, dq = states(name)
    return _stack([formulas(system, q[i], dq[i], measures(name)) for i in range(len(q))])


@functools.lru_cache(maxsize=None)
def floors(name):
    """Per array: the disagreement of the host accessors and formulas(), two independent fp64 evaluations, relative to max(1, |want|inf),
    over the system's table.  Measured on the CPU, never from the kernel."""
    ref, clo = state_references(name), state_formulas(name)
    return {f: float(np.abs(getattr(clo, f) - getattr(ref, f)).max()) / max(1.0, float(np.abs(getattr(ref, f)).max())) for f in FIELDS}


def tolerance(name, field):
    """The project's max(tolerance, 64 x floor)."""
    return max(TOL[field], 64.0 * floors(name)[field])


def segment_lengths(name):
    """[n][S] lengths of all segments of all table states, from the host frames alone."""
    system = system_of(name)[0]
    q = states(name)[0]
    out = []
    for i in range(len(q)):
        system.q = q[i]
        p = [np.asarray(f.p())[:3] for f in system.frames]
        out.append([float(np.linalg.norm(p[b] - p[a])) for m in measures(name) for a, b in zip(m[:-1], m[1:])])
    return np.array(out)


def pick(name, B, M):
    n = len(states(name)[0])
    return (np.arange(B)[:, None] + 2 * np.arange(M)[None, :]) % n


def batch_states(name, B, M):
    """Q, dQ [B][M][nq] of a launch and the table indices behind them."""
    q, dq = states(name)
    at = pick(name, B, M)
    return q[at], dq[at], at


def expected(name, at, sel=None):
    """The reference arrays of a launch whose state (b, m) is table state at[b, m], for a selection of the system's measures (default all)."""
    ref = state_references(name)
    sel = slice(None) if sel is None else np.asarray(sel, dtype=int)
    return Arrays(*[getattr(ref, f)[at][:, :, sel] for f in FIELDS])


def worst_ratio(name, got, want, fields=FIELDS):
    """max over the arrays of |got - want|inf / (tolerance max(1, |want|inf)); anything not finite in got counts as infinite."""
    worst = 0.0
    for f in fields:
        a, w = getattr(got, f), getattr(want, f)
        if a is None:
            continue
        assert a.shape == w.shape, (f, a.shape, w.shape)
        err = np.abs(a - w).max() if a.size else 0.0
        if not np.isfinite(err):
            return float("inf")
        worst = max(worst, float(err) / (tolerance(name, f) * max(1.0, float(np.abs(w).max()))))
    return worst


def compare(name, got, want, tag="", fields=FIELDS):
    """Asserts every array of got within the bounds of want; returns {field: error / bound}."""
    out = {}
    for f in fields:
        a, w = getattr(got, f), getattr(want, f)
        if a is None:
            continue
        assert a.shape == w.shape, (tag, f, a.shape, w.shape)
        assert not np.isnan(a).any(), "%s%s: %d entries not written" % (tag, f, int(np.isnan(a).sum()))
        err = float(np.abs(a - w).max()) if a.size else 0.0
        bound = tolerance(name, f) * max(1.0, float(np.abs(w).max()))
        print("%s%s: error %.3e, bound %.3e" % (tag, f, err, bound))
        assert err <= bound, (tag, f, err, bound)
        out[f] = err / bound
    return out


# ---- structure: paths, exclusive configs, exact zeros -------------------------------------------------------------------------------
def _path(system, f):
    """The joints of frame f's path, nearest the frame first: [(config index, joint frame)]."""
    place = {id(c): k for k, c in enumerate(system.configs)}
    out, frame = [], system.frames[f]
    while frame is not None:
        if frame.config is not None:
            out.append((place[id(frame.config)], frame))
        frame = frame.parent
    return out


def exclusive(system, a, b):
    """Configs on exactly one of the two paths (the reference's seg_table): the only ones that move the segment."""
    ka, kb = {k for k, _ in _path(system, a)}, {k for k, _ in _path(system, b)}
    return ka ^ kb, ka & kb


def structural_zeros(system, measure_list):
    """(zq [T][nq], zqq [T][nq][nq]): True where no segment of the measure has the config (both configs) among its exclusive ones --
    the entries of LQ and VQ (of LQQ) that are exactly 0.0."""
    nq = len(system.configs)
    zq, zqq = np.ones((len(measure_list), nq), dtype=bool), np.ones((len(measure_list), nq, nq), dtype=bool)
    for t, m in enumerate(measure_list):
        for a, b in zip(m[:-1], m[1:]):
            ex = sorted(exclusive(system, a, b)[0])
            zq[t, ex] = False
            zqq[np.ix_([t], ex, ex)] = False
    return zq, zqq


# ---- the formulas of the issue, and the mistakes ---------------------------------------------------------------------------------
def _point(system, f):
    """p_F, {k: JP_F[k]}, the path as [(k, axis a_k, rotary)] nearest the frame first."""
    p = np.asarray(system.frames[f].p())[:3]
    JP, path = {}, []
    for k, joint in _path(system, f):
        ax, rotary = fr._axis(joint)
        gK = np.asarray(joint.g())
        a, o = gK[:3, ax], gK[:3, 3]
        JP[k] = np.cross(a, p - o) if rotary else a.copy()
        path.append((k, a, rotary))
    return p, JP, path


def _second(JP, path, mutant):
    """{(j, k): P_F[j, k]} for all pairs of the path: a_near x JP[far] for a rotary near-the-world one, 0 for a prismatic one."""
    P = {}
    for n_far, (kf, af, rf) in enumerate(path):
        for kn, an, rn in path[n_far:]:                      # kn: nearer the world, or the same
            axis, rotary = an, rn
            if mutant == "descendant_axis":
                axis = af
            if mutant == "prismatic_ancestor_rotary":
                rotary = True
            v = np.cross(axis, JP[kf]) if rotary else np.zeros(3)
            if mutant == "diagonal_dropped" and kn == kf:
                v = np.zeros(3)
            P[(kn, kf)] = P[(kf, kn)] = v
    return P


def formulas(system, q, dq, measure_list, mutant=None, planted=None):
    """The five arrays from the closed formulas of the issue.  `mutant` plants one mistake; `planted` (a list) collects the size of what
    each planting changed in a term of some l_jk (d . d_jk / l, l_j l_k / l)."""
    assert mutant is None or mutant in MUTANTS
    planted = [] if planted is None else planted
    system.q, system.dq = np.asarray(q, dtype=float), np.asarray(dq, dtype=float)
    dq = np.asarray(dq, dtype=float)
    nq = len(system.configs)
    seg = []                                                   # per segment of the flat list: (l, v, l_k [nq], v_k [nq], l_jk [nq][nq])
    ranges = []
    for m in measure_list:
        m = list(m) + ([m[0]] if mutant == "closed_line" else [])
        first = len(seg)
        for a, b in zip(m[:-1], m[1:]):
            pa, JPa, path_a = _point(system, a)
            pb, JPb, path_b = _point(system, b)
            Pa, Pb = _second(JPa, path_a, mutant), _second(JPb, path_b, mutant)
            Ca, Cb = _second(JPa, path_a, None), _second(JPb, path_b, None)
            ex, common_ = exclusive(system, a, b)
            if mutant == "common_not_excluded":
                ex = ex | common_
            ex = sorted(ex)
            d = pb - pa
            with np.errstate(divide="ignore", invalid="ignore"):
                l = np.sqrt(d.dot(d))
                e = d / l
                zero = np.zeros(3)
                dk = {k: JPb.get(k, zero) - JPa.get(k, zero) for k in ex}
                lk, vk, ljk = np.zeros(nq), np.zeros(nq), np.zeros((nq, nq))
                for k in ex:
                    lk[k] = e.dot(dk[k])
                for j in ex:
                    for k in ex:
                        djk = Pb.get((j, k), zero) - Pa.get((j, k), zero)
                        if mutant in ("descendant_axis", "prismatic_ancestor_rotary", "diagonal_dropped"):
                            planted.append(abs(float(d.dot(djk - (Cb.get((j, k), zero) - Ca.get((j, k), zero))) / l)))
                        cross = lk[j] * lk[k]
                        if mutant == "ljlk_dropped":
                            planted.append(abs(float(cross / l)))
                            cross = 0.0
                        ljk[j, k] = (dk[j].dot(dk[k]) + d.dot(djk) - cross) / l
                ddot = sum((dk[k] * dq[k] for k in ex), np.zeros(3))
                for k in ex:
                    vk[k] = sum(ljk[j, k] * dq[j] for j in ex)
                seg.append((l, e.dot(ddot), lk, vk, ljk))
        ranges.append((first, len(seg)))
    T = len(measure_list)
    out = Arrays(np.zeros(T), np.zeros(T), np.zeros((T, nq)), np.zeros((T, nq)), np.zeros((T, nq, nq)))
    for t, (s0, s1) in enumerate(ranges):
        if mutant == "boundary_off_by_one":
            s1 = min(s1 + 1, len(seg))
        for s in range(s0, s1):
            for a, v in zip(out, seg[s]):
                a[t] += v
    return out


def reaches(name, mutant, state=0):
    """Does the mistake change anything on this system's table?  The structural ones from the measures; the planted terms from their size
    at the state, as the closed formulas see it (a term of some l_jk changed by 0.05 at the least)."""
    system, ms = system_of(name)[0], measures(name)
    if mutant in ("closed_line", "state_off_by_one"):
        return True
    if mutant == "boundary_off_by_one":
        return len(ms) > 1
    if mutant == "common_not_excluded":      # (a common prismatic config moves both ends by the same vector: an exact zero either way)
        rotary = {k for f in range(len(system.frames)) for k, joint in _path(system, f) if fr._axis(joint)[1]}
        return any(exclusive(system, a, b)[1] & rotary for m in ms for a, b in zip(m[:-1], m[1:]))
    q, dq = states(name)
    planted = []
    formulas(system, q[state], dq[state], ms, mutant=mutant, planted=planted)
    return bool(planted) and max(planted) >= 0.05
