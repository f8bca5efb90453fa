"""The device L-BFGS (dm_lbfgs_init / dm_lbfgs_advance / dm_lbfgs_result, csrc/dm_lbfgs_dev.h) restated one call at a time: the state
layout of lb_carve, an independent reference of ONE advance of ONE pair (dot products in np.longdouble, the direction as -H g with a
dense inverse-Hessian approximation instead of a two-loop recursion, the line search and the stopping rules from the header of
csrc/dm_lbfgs.hip), a-priori rounding bounds that mark a step "knife-edge" when a decision could go either way, the objective functions
and the harness that drives either the kernel (checking every call) or the reference alone.  A helper module, not a test file."""
import types

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of float64
C1, C2 = 1e-3, 0.9                  # strong Wolfe: sufficient decrease, curvature (SciPy's L-BFGS-B constants)

# ---------------------------------------------------------------------------------------------------------------- state layout
# float64 blocks in the order lb_carve lays them out, then the int32 block
LS_F, LS_DPHI0, LS_T, LS_TPREV, LS_FPREV, LS_DPREV, LS_TLO, LS_FLO, LS_DLO, LS_THI, LS_FHI, LS_DHI, LS_GAMMA, LS_TBEST, LS_FBEST = range(15)
LS_NSCAL = 16
LI_STATUS, LI_PHASE, LI_ITER, LI_NFEV, LI_NHIST, LI_HEAD, LI_LSIT = range(7)
LI_NINT = 8
RUN, GTOL, FTOL, MAXITER, MAXFUN, LSFAIL = range(6)
PH_FIRST, PH_BRACKET, PH_ZOOM = range(3)
EINVAL = -1

LABELS = ("bracket-accept", "extrapolate", "bracket->zoom-armijo", "bracket->zoom-slope", "zoom-hi", "zoom-lo", "zoom-accept",
          "maxls-accept", "maxls-back", "line-search-fail", "restart", "curvature-skip")
FIELDS = ("x", "g", "d", "S", "Y", "rho", "al", "sc", "ic")


def state_bytes(B, n, m):
    """what dm_lbfgs_state_bytes answers: the blocks below and 1 KiB of slack"""
    return (3 * B * n + 2 * B * m * n + 2 * B * m + LS_NSCAL * B) * 8 + LI_NINT * B * 4 + 1024


def _carve(words, B, n, m):
    """words: the state buffer as a float64 array.  Returns the blocks as copies."""
    shapes = (("x", (B, n)), ("g", (B, n)), ("d", (B, n)), ("S", (B, m, n)), ("Y", (B, m, n)), ("rho", (B, m)), ("al", (B, m)), ("sc", (B, LS_NSCAL)))
    out, p = {}, 0
    for name, shp in shapes:
        size = int(np.prod(shp))
        out[name] = words[p:p + size].reshape(shp).copy()
        p += size
    nint = B * LI_NINT
    end = p * 8 + nint * 4
    assert end <= words.size * 8, "carved end past the buffer"
    out["ic"] = words[p:p + (nint + 1) // 2].view(np.int32)[:nint].reshape(B, LI_NINT).copy()
    return out, end


def snapshot(state_tensor, B, n, m, nbytes=None):
    """the state buffer (a float64 torch tensor on the device, or a float64 NumPy array) as NumPy blocks x, g, d (B,n); S, Y (B,m,n);
    rho, al (B,m); sc (B,16); ic (B,8) int32.  nbytes: what dm_lbfgs_state_bytes(B, n, m) answered (default: the restated formula)."""
    words = state_tensor.detach().cpu().numpy() if hasattr(state_tensor, "detach") else np.asarray(state_tensor)
    assert words.dtype == np.float64 and words.ndim == 1
    out, end = _carve(words, B, n, m)
    assert end <= (state_bytes(B, n, m) if nbytes is None else nbytes), (end, nbytes)
    return types.SimpleNamespace(**out)


def pair_of(snap, b):
    return {k: getattr(snap, k)[b] for k in FIELDS}


def fresh_state(x0, m):
    """what dm_lbfgs_init leaves: everything zero, x = x0"""
    B, n = x0.shape
    z = lambda *s: np.zeros(s)
    return types.SimpleNamespace(x=x0.copy(), g=z(B, n), d=z(B, n), S=z(B, m, n), Y=z(B, m, n), rho=z(B, m), al=z(B, m), sc=z(B, LS_NSCAL),
                                 ic=np.zeros((B, LI_NINT), np.int32))


# ---------------------------------------------------------------------------------------------------------------- arithmetic
def dot_ld(a, b):
    """(a . b in longdouble, a-priori bound of a float64 evaluation in any order with or without fma: n 2^-53 sum |a_i b_i|)"""
    p = np.asarray(a, LD) * np.asarray(b, LD)
    return p.sum(), LD(p.size * U) * np.abs(p).sum()


class _Knife:
    """comparisons that remember whether the other answer lies within the rounding bound of their operands"""

    def __init__(self):
        self.why = []

    def mark(self, why):
        self.why.append(why)

    def le(self, a, b, err, why):
        if abs(a - b) <= err:
            self.why.append(why)
        return bool(a <= b)

    def ge(self, a, b, err, why):
        return self.le(b, a, err, why)

    def gt(self, a, b, err, why):
        return not self.le(a, b, err, why)


def live_rows(head, nh, m):
    """ring-buffer slots of the live history pairs, oldest first: the newest sits just behind the head"""
    return [(head - nh + j) % m for j in range(nh)]


def dense_direction(S, Y, rows, g):
    """-H g in longdouble, H the BFGS inverse-Hessian approximation built densely from the pairs (S[i], Y[i]), i in rows (oldest first):
    H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T from gamma I, gamma = s^T y / y^T y of the newest pair.  (The product is expanded
    with H symmetric: H - s u^T - u s^T, u = rho H y - (rho^2 y^T H y + rho) s / 2 -- the same matrix in O(n^2) per pair.)"""
    g = np.asarray(g, LD)
    if not rows:
        return -g
    s, y = np.asarray(S[rows[-1]], LD), np.asarray(Y[rows[-1]], LD)
    H = np.eye(g.size, dtype=LD) * ((s * y).sum() / (y * y).sum())
    for i in rows:
        s, y = np.asarray(S[i], LD), np.asarray(Y[i], LD)
        rho = LD(1) / (s * y).sum()
        Hy = np.dot(H, y)
        u = rho * Hy - (rho * rho * (y * Hy).sum() + rho) / 2 * s
        H -= np.outer(s, u)
        H -= np.outer(u, s)
    return -np.dot(H, g)


def _seq_dot(a, b):
    return np.cumsum(a * b)[-1]             # (a running sum: left to right in float64)


def two_loop_f64(history, g):
    """the ordinary two-loop recursion in float64 with sequential sums; history = (S, Y, rows) as for dense_direction.  Only used to size
    the direction tolerance: its deviation from dense_direction is what float64 costs on this history."""
    S, Y, rows = history
    q = -np.asarray(g, np.float64)
    if not rows:
        return q
    rho = {i: 1.0 / _seq_dot(S[i], Y[i]) for i in rows}
    al = {}
    for i in reversed(rows):
        al[i] = rho[i] * _seq_dot(S[i], q)
        q = q - al[i] * Y[i]
    new = rows[-1]
    q = q * (_seq_dot(S[new], Y[new]) / _seq_dot(Y[new], Y[new]))
    for i in rows:
        be = rho[i] * _seq_dot(Y[i], q)
        q = q + (al[i] - be) * S[i]
    return q


def direction_tolerance(S, Y, rows, g, dense=None):
    """(tolerance, dense direction): 8 x the largest deviation of two_loop_f64 from the dense longdouble direction (the 8 covers a tree
    against a sequential summation order and fma), at least 64 2^-53 |d|_inf"""
    dense = dense_direction(S, Y, rows, g) if dense is None else dense
    dev = float(np.abs(two_loop_f64((S, Y, rows), g).astype(LD) - dense).max())
    return max(8.0 * dev, 64.0 * U * float(np.abs(dense).max())), dense


def _interp(a, fa, da, b, fb, db, K):
    """minimiser of the cubic through (a, fa, da), (b, fb, db), else the midpoint, kept in the inner 80 % of the interval.
    Returns (t, bound of a float64 evaluation's deviation, "cubic" | "mid" | "point")."""
    a, fa, da, b, fb, db = (LD(v) for v in (a, fa, da, b, fb, db))
    if a == b:                                  # a trial on an end of the interval: the interval is that point
        return a, LD(0), "point"
    t, et, how = (a + b) / 2, 2 * U * max(a, b), "mid"
    slope = (fa - fb) / (a - b)
    d1 = da + db - 3 * slope
    e_d1 = 4 * U * (abs(da) + abs(db) + 3 * abs(slope))
    rad = d1 * d1 - da * db
    e_rad = 2 * abs(d1) * e_d1 + 3 * U * (d1 * d1 + abs(da * db))
    if np.isfinite(rad):
        if abs(rad) <= e_rad:
            K.mark("cubic discriminant")
        elif rad > 0:
            d2 = np.sqrt(rad) * (1 if b > a else -1)
            e_d2 = e_rad / (2 * np.sqrt(rad)) + U * abs(d2)
            den = db - da + 2 * d2
            e_den = 2 * e_d2 + 3 * U * (abs(db) + abs(da) + 2 * abs(d2))
            if abs(den) <= e_den:
                K.mark("cubic denominator")
            elif den != 0:
                num = db + d2 - d1
                e_num = e_d2 + e_d1 + 3 * U * (abs(db) + abs(d2) + abs(d1))
                c = b - (b - a) * num / den
                if np.isfinite(c):
                    e_c = abs(b - a) * (e_num / abs(den) + abs(num) * e_den / (den * den)) + 4 * U * (abs(b) + abs((b - a) * num / den))
                    t, et, how = c, e_c, "cubic"
    return t, et, how


def _clamp80(t, a, b):
    lo, hi = min(a, b), max(a, b)
    w = hi - lo
    return min(max(t, lo + w / 10), hi - w / 10)


def _interp_spread(lo3, hi3, which, e, K):
    """the interpolated step and the interval a float64 evaluation may land in when the slope of the point `which` ("lo" / "hi") is
    only known to +- e"""
    ts, kinds = [], set()
    for shift in (LD(0), -e, e):
        p = [list(lo3), list(hi3)]
        p[0 if which == "lo" else 1][2] = LD(p[0 if which == "lo" else 1][2]) + shift
        t, et, how = _interp(*p[0], *p[1], K)
        kinds.add(how)
        a, b = LD(lo3[0]), LD(hi3[0])
        slack = 4 * U * max(abs(a), abs(b))
        ts.append((_clamp80(t, a, b), _clamp80(t - et, a, b) - slack, _clamp80(t + et, a, b) + slack))
    if len(kinds) > 1:
        K.mark("cubic or bisection")
    return ts[0][0], min(v[1] for v in ts), max(v[2] for v in ts)


# ---------------------------------------------------------------------------------------------------------------- one advance
def reference_step(snap_before, xt, f, g, opts):
    """The expected result of one dm_lbfgs_advance for one pair.  snap_before: the pair's blocks (pair_of); xt, f, g: the trial point that
    was evaluated, its energy and gradient; opts: m, ftol, pgtol, maxiter, maxfun, maxls.
    Returns a namespace: kind ("idle" | "trial" | "fail" | "restart" | "stop" | "direction"), labels, knife (list of reasons: not empty =
    some decision lies within the rounding bound of its operands), ic (expected integers, -1 = not part of the contract: phase and
    line-search count of a pair that stopped), after (the pair's blocks as the reference computes them), xt (its next trial point),
    t_lo / t_hi (where a float64 evaluation of the next step length may land), accepted, updated (history pair stored as live),
    rho_tol / gamma_tol (relative)."""
    o = opts
    m = int(o["m"])
    s = snap_before
    K = _Knife()
    after = {k: np.array(v, copy=True) for k, v in s.items()}
    sc, ic = after["sc"], after["ic"]
    xt = np.asarray(xt, np.float64)
    g = np.asarray(g, np.float64)
    exp = types.SimpleNamespace(kind="idle", labels=[], knife=K.why, ic=ic.copy(), after=after, xt=xt.copy(), t_lo=None, t_hi=None,
                                accepted=False, updated=False, rho_tol=0.0, gamma_tol=0.0, rows=None, dense=None)
    if ic[LI_STATUS] != RUN:
        return exp
    phase, nfev = int(ic[LI_PHASE]), int(ic[LI_NFEV]) + 1
    f0 = LD(sc[LS_F])
    ft = LD(f)
    finite = bool(np.isfinite(ft))
    restart = False
    if phase != PH_FIRST:
        # ---------------------------------------------------------------------------------------- the line search sees a new trial
        tt, dphi0 = LD(sc[LS_T]), LD(sc[LS_DPHI0])
        lsit = int(ic[LI_LSIT]) + 1
        rhs = f0 + LD(C1) * tt * dphi0
        armijo = finite and K.le(ft, rhs, 4 * np.spacing(np.float64(abs(rhs))), "sufficient decrease")
        dphit, e = dot_ld(g, s["d"])          # (without sufficient decrease the slope is stored with the point and never compared)
        d64 = np.float64(dphit)
        if armijo and ft < LD(sc[LS_FBEST]):
            sc[LS_FBEST], sc[LS_TBEST] = f, sc[LS_T]
        wolfe = lambda: K.le(abs(dphit), -LD(C2) * dphi0, e + 2 * U * abs(dphi0), "curvature condition")
        cur = (sc[LS_T], np.float64(f), d64)
        prev = (sc[LS_TPREV], sc[LS_FPREV], sc[LS_DPREV])
        decided, tn, t_lo, t_hi = None, None, None, None

        def put(slot, v):
            sc[slot], sc[slot + 1], sc[slot + 2] = v

        def interp(which):
            lo3 = (sc[LS_TLO], sc[LS_FLO], sc[LS_DLO])
            hi3 = (sc[LS_THI], sc[LS_FHI], sc[LS_DHI])
            if not np.isfinite(sc[LS_FHI]):
                mid = (LD(lo3[0]) + LD(hi3[0])) / 2
                return mid, mid - 2 * U * abs(mid), mid + 2 * U * abs(mid)
            return _interp_spread(lo3, hi3, which, e if armijo else LD(0), K)

        if phase == PH_BRACKET:
            if not armijo or (lsit > 1 and ft >= LD(sc[LS_FPREV])):
                exp.labels.append("bracket->zoom-armijo")
                put(LS_TLO, prev), put(LS_THI, cur)
                ic[LI_PHASE] = PH_ZOOM
                tn, t_lo, t_hi = interp("hi")
            elif wolfe():
                exp.labels.append("bracket-accept")
                decided = "accept"
            elif K.ge(dphit, LD(0), e, "sign of the slope"):
                exp.labels.append("bracket->zoom-slope")
                put(LS_TLO, cur), put(LS_THI, prev)
                ic[LI_PHASE] = PH_ZOOM
                tn, t_lo, t_hi = interp("lo")
            else:
                exp.labels.append("extrapolate")
                put(LS_TPREV, cur)
                tn = LD(np.float64(2.5) * sc[LS_T])
                t_lo = t_hi = tn
        else:
            moved = "hi"
            if not armijo or ft >= LD(sc[LS_FLO]):
                exp.labels.append("zoom-hi")
                put(LS_THI, cur)
            elif wolfe():
                exp.labels.append("zoom-accept")
                decided = "accept"
            else:
                exp.labels.append("zoom-lo")
                width = LD(sc[LS_THI]) - LD(sc[LS_TLO])
                if K.ge(dphit * width, LD(0), e * abs(width), "side of the minimum"):
                    put(LS_THI, (sc[LS_TLO], sc[LS_FLO], sc[LS_DLO]))
                put(LS_TLO, cur)
                moved = "lo"
            if decided is None:
                tn, t_lo, t_hi = interp(moved)
                a, b = LD(sc[LS_TLO]), LD(sc[LS_THI])
                big = max(abs(a), abs(b))
                if K.le(abs(b - a), LD(1e-14) * big, 4 * U * big * LD(1e-14) + 2 * U * abs(b - a), "collapsed interval"):
                    decided = "accept" if armijo else "fail"
        if decided is None and lsit >= int(o["maxls"]):
            # out of trials: the best step with sufficient decrease -- this one, or one more evaluation there
            if sc[LS_TBEST] > 0.0 and sc[LS_TBEST] == sc[LS_T]:
                exp.labels.append("maxls-accept")
                decided = "accept"
            elif sc[LS_TBEST] > 0.0:
                exp.labels.append("maxls-back")
                tn = t_lo = t_hi = LD(sc[LS_TBEST])
                ic[LI_LSIT] = int(o["maxls"]) - 1
            else:
                decided = "fail"
        elif decided is None:
            ic[LI_LSIT] = lsit
        if decided is None and nfev >= int(o["maxfun"]):
            decided = "accept" if armijo else "fail"
        if decided is None:
            exp.kind = "trial"
            t64 = np.float64(tn)
            sc[LS_T] = t64
            ic[LI_NFEV] = nfev
            exp.xt = np.asarray(s["x"].astype(LD) + LD(t64) * s["d"].astype(LD), np.float64)
            exp.t_lo, exp.t_hi = t_lo, t_hi
            exp.ic = ic.copy()
            return exp
        if decided == "fail":
            if ic[LI_NHIST] == 0:
                exp.kind = "fail"
                exp.labels.append("line-search-fail")
                ic[LI_NFEV], ic[LI_STATUS] = nfev, LSFAIL
                exp.xt = s["x"].copy()
                exp.ic = ic.copy()
                exp.ic[LI_PHASE] = exp.ic[LI_LSIT] = -1
                return exp
            exp.labels.append("restart")
            restart = True
    # -------------------------------------------------------------------------------------------- the trial point is accepted
    nh, head, it = int(ic[LI_NHIST]), int(ic[LI_HEAD]), int(ic[LI_ITER])
    if restart:
        nh = 0
        fcur = sc[LS_F]
        gacc = s["g"]
    else:
        exp.accepted = True
        if phase != PH_FIRST:
            sv, yv = xt - s["x"], g - s["g"]                      # (float64 subtraction is correctly rounded: these are the stored rows)
            after["S"][head], after["Y"][head] = sv, yv
            sy, e_sy = dot_ld(sv, yv)
            yy, e_yy = dot_ld(yv, yv)
            if yy > 0 and K.gt(sy, LD(2.2e-16) * yy, e_sy + LD(2.2e-16) * (e_yy + U * yy), "curvature of the new pair"):
                exp.updated = True
                after["rho"][head] = np.float64(1 / sy)
                sc[LS_GAMMA] = np.float64(sy / yy)
                exp.rho_tol = float(e_sy / abs(sy)) + 2 * U
                exp.gamma_tol = float(e_sy / abs(sy) + e_yy / yy) + 2 * U
                head = (head + 1) % m
                nh = min(nh + 1, m)
            else:
                exp.labels.append("curvature-skip")
            it += 1
        after["x"][:], after["g"][:] = xt, g
        gacc = g
        fcur = np.float64(f)
        gmax = np.inf if np.isnan(g).any() else float(np.abs(g).max())
        status = RUN
        if not finite or not np.isfinite(gmax):
            status = LSFAIL
        elif gmax <= float(o["pgtol"]):                                  # (a maximum of float64 numbers: nothing is rounded)
            status = GTOL
        elif phase != PH_FIRST and K.le(f0 - ft, LD(o["ftol"]) * max(abs(f0), abs(ft), LD(1)),
                                         2 * U * (abs(f0 - ft) + LD(o["ftol"]) * max(abs(f0), abs(ft), LD(1))), "ftol test"):
            status = FTOL
        elif it >= int(o["maxiter"]):
            status = MAXITER
        elif nfev >= int(o["maxfun"]):
            status = MAXFUN
        if status != RUN:
            exp.kind = "stop"
            sc[LS_F] = f
            ic[LI_STATUS], ic[LI_ITER], ic[LI_NFEV], ic[LI_NHIST], ic[LI_HEAD] = status, it, nfev, nh, head
            exp.xt = xt.copy()
            exp.ic = ic.copy()
            exp.ic[LI_PHASE] = exp.ic[LI_LSIT] = -1
            return exp
    # -------------------------------------------------------------------------------------------- new direction and first step
    exp.kind = "restart" if restart else "direction"
    rows = live_rows(head, nh, m)
    d = dense_direction(after["S"], after["Y"], rows, gacc)
    exp.rows, exp.dense = rows, d
    dphi0, e0 = dot_ld(gacc, d)
    if not K.le(dphi0, -e0, e0, "descent direction"):           # numerical breakdown: steepest descent, history dropped
        K.mark("not a descent direction")
        d = -np.asarray(gacc, LD)
        dphi0, nh = dot_ld(gacc, d)[0], 0
    t0, r = LD(1), 0.0
    if it == 0 or restart:
        dn = np.sqrt((d * d).sum())
        if dn > 0:
            r = (d.size / 2 + 4) * U
            if abs(dn - 1) <= r:
                K.mark("first step at |d| = 1")
            t0 = min(LD(1), 1 / dn)
    exp.t_lo, exp.t_hi = t0 * (1 - r), min(LD(1), t0 * (1 + r))
    after["d"][:] = np.asarray(d, np.float64)
    t64 = np.float64(t0)
    exp.xt = np.asarray(after["x"].astype(LD) + LD(t64) * after["d"].astype(LD), np.float64)
    sc[LS_F], sc[LS_DPHI0], sc[LS_T] = fcur, np.float64(dphi0), t64
    sc[LS_TPREV], sc[LS_FPREV], sc[LS_DPREV] = 0.0, fcur, np.float64(dphi0)
    sc[LS_TBEST], sc[LS_FBEST] = 0.0, fcur
    ic[LI_PHASE], ic[LI_ITER], ic[LI_NFEV], ic[LI_NHIST], ic[LI_HEAD], ic[LI_LSIT] = PH_BRACKET, it, nfev, nh, head, 0
    exp.ic = ic.copy()
    return exp


# ---------------------------------------------------------------------------------------------------------------- the check of one call
def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_step(before, after, xt_before, xt_after, g_up, exp, m, stats):
    """one pair, one call: the kernel's state after the call against the expectation (what is compared is listed in the docstring of
    tests/test_gpu_lbfgs.py::test_every_call_against_the_reference).  A knife-edge step is counted and not judged."""
    if exp.kind == "idle":
        for k in FIELDS:
            assert _same(before[k], after[k]), f"finished pair: {k} changed"
        assert _same(xt_before, xt_after), "finished pair: trial point changed"
        return
    stats["steps"] += 1
    if exp.knife:
        stats["knife"] += 1
        stats["why"].extend(exp.knife)
        return
    got = after["ic"][:7].astype(int)
    want = exp.ic[:7].astype(int)
    ok = (want < 0) | (got == want)
    assert ok.all(), f"integer state {got.tolist()} expected {want.tolist()} ({exp.kind}, {exp.labels})"
    sca = after["sc"]
    head0 = int(before["ic"][LI_HEAD])
    if exp.accepted:
        assert _same(after["x"], xt_before), "x is not the accepted trial point"
        assert _same(after["g"], g_up), "g is not the uploaded gradient"
        assert _same(sca[LS_F:LS_F + 1], exp.after["sc"][LS_F:LS_F + 1]), "stored energy is not the uploaded one"
        if before["ic"][LI_PHASE] != PH_FIRST:
            assert _same(after["S"][head0], xt_before - before["x"]) and _same(after["Y"][head0], g_up - before["g"]), "new history row"
            keep = [i for i in range(m) if i != head0]
            assert _same(after["S"][keep], before["S"][keep]) and _same(after["Y"][keep], before["Y"][keep]), "another history row changed"
            assert _same(after["rho"][keep], before["rho"][keep])
            if exp.updated:
                r_ref, g_ref = exp.after["rho"][head0], exp.after["sc"][LS_GAMMA]
                assert abs(after["rho"][head0] - r_ref) <= exp.rho_tol * abs(r_ref), ("rho", after["rho"][head0], r_ref, exp.rho_tol)
                assert abs(sca[LS_GAMMA] - g_ref) <= exp.gamma_tol * abs(g_ref), ("gamma", sca[LS_GAMMA], g_ref, exp.gamma_tol)
            else:
                assert after["rho"][head0] == before["rho"][head0] and sca[LS_GAMMA] == before["sc"][LS_GAMMA], "skipped pair left a trace"
        else:
            assert _same(after["S"], before["S"]) and _same(after["Y"], before["Y"]) and _same(after["rho"], before["rho"])
    else:
        for k in ("x", "g", "S", "Y", "rho"):
            assert _same(before[k], after[k]), f"{exp.kind}: {k} changed"
    if exp.kind in ("stop", "fail"):
        assert _same(xt_after, after["x"]), "a stopped pair's trial point is its iterate"
        if exp.kind == "stop":
            assert _same(after["d"], before["d"])
        return
    if exp.kind == "trial":
        assert _same(after["d"], before["d"]), "direction changed inside a line search"
        t = LD(sca[LS_T])
        span = 4 * U * abs(t)
        assert exp.t_lo - span <= t <= exp.t_hi + span, f"step {float(t)!r} outside [{float(exp.t_lo)!r}, {float(exp.t_hi)!r}] ({exp.labels})"
        tt = before["sc"][LS_T]
        if "zoom-hi" in exp.labels or "bracket->zoom-armijo" in exp.labels:
            assert sca[LS_THI] == tt
        if "zoom-lo" in exp.labels or "bracket->zoom-slope" in exp.labels:
            assert sca[LS_TLO] == tt
        if "bracket->zoom-armijo" in exp.labels:
            assert sca[LS_TLO] == before["sc"][LS_TPREV]
        if "extrapolate" in exp.labels:
            assert sca[LS_TPREV] == tt
    else:
        # new direction: against the dense longdouble -H g of the kernel's own stored history
        rows = live_rows(int(after["ic"][LI_HEAD]), int(after["ic"][LI_NHIST]), m)
        # (the rows and the gradient are bit for bit the reference's by the assertions above: its dense direction is this one's)
        same = rows == exp.rows and _same(after["S"], exp.after["S"]) and _same(after["Y"], exp.after["Y"]) and _same(after["g"], exp.after["g"])
        tol, dense = direction_tolerance(after["S"], after["Y"], rows, after["g"], exp.dense if same else None)
        err = float(np.abs(after["d"].astype(LD) - dense).max())
        stats["ratio"] = max(stats["ratio"], 8.0 * err / tol)
        assert err <= tol, f"direction off by {err:.3e}, tolerance {tol:.3e} (history {len(rows)})"
        if exp.kind == "restart":
            assert _same(after["d"], -before["g"]) and sca[LS_F] == before["sc"][LS_F]
        dphi0, e0 = dot_ld(after["g"], after["d"])
        assert abs(LD(sca[LS_DPHI0]) - dphi0) <= e0, "slope at the start of the line search"
        t = LD(sca[LS_T])
        assert exp.t_lo <= t <= exp.t_hi, f"first step {float(t)!r} outside [{float(exp.t_lo)!r}, {float(exp.t_hi)!r}]"
        assert sca[LS_TPREV] == 0.0 and sca[LS_TBEST] == 0.0 and sca[LS_FPREV] == sca[LS_F] and sca[LS_FBEST] == sca[LS_F]
    want_xt = after["x"].astype(LD) + LD(sca[LS_T]) * after["d"].astype(LD)
    assert (np.abs(xt_after.astype(LD) - want_xt) <= np.spacing(np.abs(xt_after))).all(), "next trial point is not x + t d"


# ---------------------------------------------------------------------------------------------------------------- objective functions
# each is one pair's function (x (n,), number of accepted iterates) -> (energy, gradient (n,)) in float64
def quadratic(n, seed, cond=1e3, origin=0.0, centred=False):
    """z^T A z / 2 - b^T z, z = x - origin, with eigenvalues 1 .. cond (geometric) in a random basis and a known minimiser fn.xstar
    (the energy at the origin is exactly 0: along a direction that climbs from there, no trial's energy drowns in the rounding of f0).
    centred: the same function plus a constant, evaluated as r^T A r / 2, r = x - xstar -- its minimum is 0, so the decrease of a step
    near the minimiser is not lost in the rounding of an energy of size 1e4 and the gradient test can be as tight as 1e-8"""
    rng = np.random.default_rng(seed)
    lam = np.geomspace(1.0, cond, n) if n > 1 else np.ones(1)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * lam) @ Q.T
    A = (A + A.T) / 2
    xs = rng.uniform(-1.0, 1.0, n)
    b = A @ xs

    def fn(x, nit=0):
        z = x - origin - (xs if centred else 0.0)
        Az = A @ z
        return (0.5 * float(z @ Az), Az) if centred else (0.5 * float(z @ Az) - float(b @ z), Az - b)
    fn.xstar, fn.lam_min = xs + origin, float(lam.min())
    return fn


def rosenbrock(x, nit=0):
    import scipy.optimize
    return float(scipy.optimize.rosen(x)), scipy.optimize.rosen_der(x)


def barrier(c):
    """sum c_i (x_i - log x_i): not a number outside x > 0, minimiser at 1"""
    c = np.asarray(c, np.float64)

    def fn(x, nit=0):
        with np.errstate(all="ignore"):
            if not (x > 0).all():
                return float("nan"), c * (1.0 - 1.0 / x)
            return float((c * (x - np.log(x))).sum()), c * (1.0 - 1.0 / x)
    fn.xstar = np.ones(c.size)
    return fn


def bump(x, nit=0):
    e = float(np.exp(-0.5 * x[0] * x[0]))
    return -e, np.array([x[0] * e])


def flipped(fn):
    """the true energy with the negated gradient: every "descent" direction climbs"""
    def flip(x, nit=0):
        f, g = fn(x, nit)
        return f, -g
    return flip


def trap(fn, k):
    """the true function until k iterates have been accepted, then f + 1e3 at every new point"""
    def trapped(x, nit=0):
        f, g = fn(x, nit)
        return (f + 1e3, g) if nit >= k else (f, g)
    return trapped


def evaluate(funs, X, nit, status):
    """energies (B,) and gradients (B,n) at the trial points; finished pairs get NaN (the kernel must not look at them)"""
    B, n = X.shape
    f, g = np.full(B, np.nan), np.full((B, n), np.nan)
    for b in range(B):
        if status[b] == RUN:
            f[b], g[b] = funs[b](X[b], int(nit[b]))
    return f, g


# ---------------------------------------------------------------------------------------------------------------- the harness
def new_stats():
    return {"steps": 0, "knife": 0, "ratio": 0.0, "why": []}


def drive(eng, fun, x0, m, opts, check=True, cap=120, stats=None):
    """Run the optimiser one call at a time.  eng: a MatchEngine (the kernel runs, and with check=True every call of every pair is
    checked against reference_step started from the kernel's own state) or None (the reference alone carries the state).
    fun: one function per pair.  opts: ftol, pgtol, maxiter, maxfun, maxls.  cap: evaluations after which a running pair is a failure.
    The branch labels of a call are the reference's; on the device the exact match of phase, line-search count, iteration count and
    status, the step length and the end of the bracket that moved tie the kernel's call to the same branch.
    Returns x, f, status, nit, nfev, nhist (per pair), labels (set over all pairs), trace (per pair: one label list per call),
    energies (per pair: every energy the optimiser was given), evaluations."""
    x0 = np.ascontiguousarray(x0, np.float64)
    B, n = x0.shape
    o = dict(opts, m=m)
    stats = new_stats() if stats is None else stats
    trace, energies = [[] for _ in range(B)], [[] for _ in range(B)]
    if eng is None:
        snap, xt = fresh_state(x0, m), x0.copy()
        read = lambda: snap
        trial = lambda: xt
    else:
        import torch
        from densematcher_amd.engine import _ptr
        nbytes = int(eng.lib.dm_lbfgs_state_bytes(B, n, m))
        assert nbytes == state_bytes(B, n, m)
        state = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=eng.device)
        xtd = torch.empty((B, n), dtype=torch.float64, device=eng.device)
        x0d = eng._dev(x0, torch.float64, "x0")
        eng._chk(eng.lib.dm_lbfgs_init(eng.ctx, B, n, m, _ptr(x0d), _ptr(state), _ptr(xtd)))
        n_f64 = 3 * B * n + 2 * B * m * n + 2 * B * m + LS_NSCAL * B
        ints = state[n_f64:n_f64 + (LI_NINT * B * 4 + 7) // 8].view(torch.int32)[:LI_NINT * B].view(B, LI_NINT)
        if check:
            read = lambda: snapshot(state, B, n, m, nbytes)
        else:
            read = lambda: types.SimpleNamespace(ic=ints.cpu().numpy())
        trial = lambda: xtd.cpu().numpy()
    before, xb = read(), trial()
    if eng is not None and check:
        fr = fresh_state(x0, m)
        assert all(_same(getattr(before, k), getattr(fr, k)) for k in FIELDS) and _same(xb, x0), "dm_lbfgs_init"
    nev = 0
    while (before.ic[:, LI_STATUS] == RUN).any():
        assert nev < cap, f"still running after {cap} evaluations: status {before.ic[:, LI_STATUS].tolist()}"
        f, g = evaluate(fun, xb, before.ic[:, LI_ITER], before.ic[:, LI_STATUS])
        nev += 1
        for b in range(B):
            if before.ic[b, LI_STATUS] == RUN:
                energies[b].append(f[b])
        if eng is not None:
            fd, gd = torch.from_numpy(f).to(eng.device), torch.from_numpy(g).to(eng.device)
            eng._chk(eng.lib.dm_lbfgs_advance(eng.ctx, B, n, m, _ptr(state), _ptr(fd), _ptr(gd), _ptr(xtd), float(o["ftol"]), float(o["pgtol"]),
                                              int(o["maxiter"]), int(o["maxfun"]), int(o["maxls"])))
            after, xa = read(), trial()
            if check:
                for b in range(B):
                    pb, pa = pair_of(before, b), pair_of(after, b)
                    exp = reference_step(pb, xb[b], f[b], g[b], o)
                    check_step(pb, pa, xb[b], xa[b], g[b], exp, m, stats)
                    if exp.kind != "idle":
                        trace[b].append(["knife-edge"] if exp.knife else exp.labels)
        else:
            xa = xb.copy()
            for b in range(B):
                exp = reference_step(pair_of(snap, b), xb[b], f[b], g[b], o)
                if exp.kind == "idle":
                    continue
                stats["steps"] += 1
                stats["knife"] += bool(exp.knife)
                trace[b].append(exp.labels)
                for k in FIELDS:
                    getattr(snap, k)[b] = exp.after[k]
                xa[b] = exp.xt
            xt = xa
            after = snap
        before, xb = after, xa
    if eng is None:
        x, fo, info = snap.x.copy(), snap.sc[:, LS_F].copy(), snap.ic[:, [LI_STATUS, LI_ITER, LI_NFEV, LI_NHIST]].copy()
    else:
        xo = torch.empty((B, n), dtype=torch.float64, device=eng.device)
        fod = torch.empty((B,), dtype=torch.float64, device=eng.device)
        infod = torch.empty((B, 4), dtype=torch.int32, device=eng.device)
        eng._chk(eng.lib.dm_lbfgs_result(eng.ctx, B, n, m, _ptr(state), _ptr(xo), _ptr(fod), _ptr(infod)))
        x, fo, info = xo.cpu().numpy(), fod.cpu().numpy(), infod.cpu().numpy()
        if check:
            assert _same(x, before.x) and _same(fo, before.sc[:, LS_F].copy()), "dm_lbfgs_result"
            assert np.array_equal(info, before.ic[:, [LI_STATUS, LI_ITER, LI_NFEV, LI_NHIST]])
        assert _same(xb, x), "a stopped pair's trial point is its iterate"
    labels = {l for t in trace for call in t for l in call}
    return types.SimpleNamespace(x=x, f=fo, status=info[:, 0], nit=info[:, 1], nfev=info[:, 2], nhist=info[:, 3], labels=labels, trace=trace,
                                 energies=energies, evaluations=nev, stats=stats)


# ---------------------------------------------------------------------------------------------------------------- shared cases
TIGHT = dict(ftol=1e-15, pgtol=1e-8, maxiter=15000, maxfun=15000, maxls=20)
# the centred quadratics of the end-result tests.  ftol = 0: only the gradient test may stop them, and |g|_inf <= pgtol gives
# |x - x*|_2 <= sqrt(n) pgtol / lambda_min = 2.3e-7 at n = 513: two such minimisers are within 1e-6 of each other
QUAD = dict(TIGHT, ftol=0.0, pgtol=1e-8)
# the barrier's energy at its minimiser is 3003, one ulp of it 4.5e-13: ftol 3003 = 3e-9 is a decrease the energy can still show
BARRIER = dict(TIGHT, ftol=1e-12)
BARRIER_C = np.linspace(1.0, 1000.0, 6)


def rosen_x0(n):
    return np.tile([-1.2, 1.0], (n + 1) // 2)[:n]


# (n, m): (maxiter, maxfun) of the single-step check -- every run ends within 120 evaluations; the limits of the large shapes keep the
# dense n x n longdouble reference to a few seconds (m = 32 / 33 still run past one wrap of the ring buffer)
STEP_SHAPES = {(1, 1): (100, 110), (2, 3): (100, 110), (63, 10): (100, 110), (64, 10): (100, 110), (65, 10): (100, 110), (225, 10): (100, 60),
               (256, 32): (36, 60), (256, 33): (36, 60), (257, 10): (100, 50), (300, 5): (100, 60), (513, 64): (12, 30)}


def step_problem(n, m):
    """the three pairs of the single-step check at one shape: (functions, starts (3,n), options)"""
    if n == 1:
        funs, x0 = [quadratic(1, 11), bump, barrier([5.0])], np.array([[0.0], [2.0], [3.0]])
    else:
        funs = [quadratic(n, 7 * n + m), rosenbrock, barrier(np.linspace(1.0, 1000.0, n))]
        x0 = np.stack([np.zeros(n), rosen_x0(n), np.full(n, 3.0)])
    maxiter, maxfun = STEP_SHAPES[(n, m)]
    return funs, x0, dict(ftol=1e-12, pgtol=1e-6, maxiter=maxiter, maxfun=maxfun, maxls=20)


# fixed starts of the branch-coverage set: Rosenbrock (n, start, maxls); the first two run out of trials and fall back to the best step
FALLBACK_STARTS = [(2, (1.375, -0.304), 3), (2, (-0.708, 1.963), 2)]
COVER_STARTS = FALLBACK_STARTS + [(n, tuple(rosen_x0(n)), ls) for n in (2, 4, 10) for ls in (2, 3, 20)] + \
    [(2, (-1.9, 2.0), 20), (4, (0.5, -1.5, 2.0, -0.5), 3), (10, tuple(np.linspace(-2.0, 2.0, 10)), 2)]


def coverage_runs(eng=None, stats=None):
    """the fixed set over which every branch label must occur, on the device (eng) or by the reference alone: returns the labels seen"""
    labels = set()
    for n, start, maxls in COVER_STARTS:
        labels |= drive(eng, [rosenbrock], np.array([start]), 10, dict(TIGHT, maxls=maxls, maxfun=400), cap=401, stats=stats).labels
    q = quadratic(7, seed=2, origin=0.5)
    labels |= drive(eng, [flipped(q)], np.full((1, 7), 0.5), 10, TIGHT, cap=30, stats=stats).labels
    labels |= drive(eng, [trap(rosenbrock, 3)], rosen_x0(10)[None], 10, TIGHT, cap=80, stats=stats).labels
    labels |= drive(eng, [bump], np.array([[2.0]]), 10, dict(TIGHT, maxls=1, maxiter=1), cap=5, stats=stats).labels
    labels |= drive(eng, [barrier(BARRIER_C)], np.full((1, 6), 3.0), 10, BARRIER, cap=200, stats=stats).labels
    return labels
