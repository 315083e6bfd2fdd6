"""numpy restatement of the oracle's trust-region loop (oracle/ea_oracle.c, ea_oracle_solve_terms with the LM strategy and the
Cholesky solver) on the REDUCED system: the tangent coordinates held constant are removed from the program, as Ceres removes
constant parameter blocks and the constant components of a SubsetParameterization.  The oracle supplies the evaluations.

Everything that touches the linear system works on the m free coordinates only: Jacobi scaling, the LM diagonal, the
factorisation, the model cost change.  The step is lifted to a 6-vector with zeros at the held coordinates before Plus().
x_norm covers the ambient coordinates of the non-constant blocks.  With nothing held it is the oracle's loop statement for
statement (tests/test_constant_parameters_host.py checks that it reproduces OracleProblem.solve)."""
import numpy as np

DEFAULTS = dict(max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
                initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                max_num_consecutive_invalid_steps=5, jacobi_scaling=1)

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2


def _cholesky_solve(A, D, g):
    """(A + diag(D^2)) y = g, the oracle's solve_cholesky6 for any size; None on failure"""
    m = len(g)
    L = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            s = A[i, j] + (D[i] * D[i] if i == j else 0.0)
            for k in range(j):
                s -= L[i, k] * L[j, k]
            if i == j:
                if not s > 0.0:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    z = np.zeros(m)
    for i in range(m):
        s = g[i]
        for k in range(i):
            s -= L[i, k] * z[k]
        z[i] = s / L[i, i]
    y = np.zeros(m)
    for i in range(m - 1, -1, -1):
        s = z[i]
        for k in range(i + 1, m):
            s -= L[k, i] * y[k]
        y[i] = s / L[i, i]
    return y if np.all(np.isfinite(y)) else None


def _ldl_solve(A, D2, g):
    """(A + diag(D2)) y = g by the square-root-free factorisation A + D2 = L diag(d) L^T in the operation order of the
    product's solve_spd6 (ea_lm.h), for any size; None on failure.  Same mathematics as _cholesky_solve, other rounding."""
    m = len(g)
    L, M, inv = np.zeros((m, m)), np.zeros((m, m)), np.zeros(m)
    for j in range(m):
        d = A[j, j] + D2[j]
        for k in range(j):
            d -= L[j, k] * M[j, k]
        if not d > 0.0:
            return None
        inv[j] = 1.0 / d
        for i in range(j + 1, m):
            t = A[j, i]
            for k in range(j):
                t -= M[i, k] * L[j, k]
            M[i, j] = t
            L[i, j] = t * inv[j]
    z = np.zeros(m)
    for i in range(m):
        s = g[i]
        for k in range(i):
            s -= L[i, k] * z[k]
        z[i] = s
    y = np.zeros(m)
    for i in range(m - 1, -1, -1):
        s = z[i] * inv[i]
        for k in range(i + 1, m):
            s -= L[k, i] * y[k]
        y[i] = s
    return y if np.all(np.isfinite(y)) else None


def x_norm_of(x, held):
    use_q = not all(held[:3])
    use_t = not all(held[3:])
    return float(np.sqrt(sum(x[i] * x[i] for i in range(7) if (use_q if i < 4 else use_t))))


def solve(evaluate, quat_plus, q, t, held=(0, 0, 0, 0, 0, 0), product_rounding=False, **opts):
    """evaluate(q, t) -> dict(cost, JtJ 6x6, Jtr 6, n_invalid); quat_plus(q, delta3) -> q'.  Returns q, t, summary (the
    oracle's summary keys that the tests compare).
    product_rounding: the linear solve and the model cost change in the product's operation order instead of the oracle's
    (square-root-free factorisation with D^2 = diagonal * (1 / radius); -(g.s + (sum_a s_a A_aa s_a + 2 sum_{a<b} s_a A_ab
    s_b) / 2)).  The same loop and the same mathematics; what differs is the last bit of a step.  A test uses it to tell a
    rounding difference between the two restatements from a difference in logic."""
    o = dict(DEFAULTS)
    o.update(opts)
    held = [bool(h) for h in held]
    free = [i for i in range(6) if not held[i]]
    m = len(free)

    def plus7(x, delta):
        return np.concatenate([quat_plus(x[:4], delta[:3]), x[4:] + delta[3:]])

    def usable(e):
        return e["n_invalid"] == 0 and abs(e["cost"]) <= np.finfo(np.float64).max

    def grad_max(x, Jtr):
        neg = np.zeros(6)
        neg[free] = -Jtr[free]
        return float(np.max(np.abs(x - plus7(x, neg))))

    x = np.concatenate([np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)])
    s = dict(num_iterations=0, num_successful_steps=0, num_unsuccessful_steps=0, it_cost=[], it_radius=[], it_successful=[],
             it_gradient_max_norm=[])
    e = evaluate(x[:4], x[4:])
    if not usable(e):
        s.update(termination=FAILURE, why="initial_eval_failed")
        return x[:4].copy(), x[4:].copy(), s
    x_cost = e["cost"]
    s["initial_cost"] = x_cost
    if m == 0:  # Ceres: "no non-constant parameter blocks"
        s.update(termination=CONVERGENCE, why="function_tolerance", final_cost=x_cost, it_cost=[x_cost])
        return x[:4].copy(), x[4:].copy(), s
    JtJ, Jtr = np.asarray(e["JtJ"]), np.asarray(e["Jtr"])
    S = np.ones(m)
    if o["jacobi_scaling"]:
        S = np.array([1.0 / (1.0 + np.sqrt(JtJ[i, i])) for i in free])

    def scale(JtJ, Jtr):
        A = np.array([[JtJ[a, b] * S[ia] * S[ib] for ib, b in enumerate(free)] for ia, a in enumerate(free)])
        g = np.array([Jtr[a] * S[ia] for ia, a in enumerate(free)])
        return A, g

    A, g = scale(JtJ, Jtr)
    x_norm = x_norm_of(x, held)
    radius, decrease_factor, reuse_diagonal = o["initial_trust_region_radius"], 2.0, False
    diagonal = np.zeros(m)
    it = 0
    it_cost, it_radius, it_ok, it_g, it_dc = [x_cost], [radius], [1], [grad_max(x, Jtr)], [0.0]
    invalid = 0
    while True:
        if it >= o["max_num_iterations"]:
            term, why = NO_CONVERGENCE, "max_iterations"; break
        if it_g[it] <= o["gradient_tolerance"]:
            term, why = CONVERGENCE, "gradient_tolerance"; break
        if radius <= o["min_trust_region_radius"]:
            term, why = CONVERGENCE, "min_trust_region_radius"; break
        it += 1
        it_g.append(it_g[it - 1]); it_cost.append(x_cost); it_radius.append(radius); it_ok.append(0); it_dc.append(0.0)
        if not reuse_diagonal:
            diagonal = np.array([min(max(A[i, i], o["min_lm_diagonal"]), o["max_lm_diagonal"]) for i in range(m)])
        if product_rounding:
            y = _ldl_solve(A, diagonal * (1.0 / radius), g)
        else:
            y = _cholesky_solve(A, np.sqrt(diagonal / radius), g)
        reuse_diagonal = True
        step_ok = y is not None
        if step_ok:
            step = -y
            gs, sAs = 0.0, 0.0
            for a in range(m):
                gs += g[a] * step[a]
                for b in range(m):
                    sAs += step[a] * A[a, b] * step[b]
            if product_rounding:
                dg, off = 0.0, 0.0
                for a in range(m):
                    dg += step[a] * A[a, a] * step[a]
                    for b in range(a + 1, m):
                        off += step[a] * A[a, b] * step[b]
                sAs = dg + 2.0 * off
            model_cost_change = -(gs + 0.5 * sAs)
            step_ok = model_cost_change > 0.0
        if not step_ok:
            s["num_unsuccessful_steps"] += 1
            invalid += 1
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                term, why = FAILURE, "too_many_invalid_steps"; break
            radius *= 0.5
            continue
        invalid = 0
        delta = np.zeros(6)
        delta[free] = step * S
        cand = plus7(x, delta)
        ec = evaluate(cand[:4], cand[4:])
        cand_cost = ec["cost"] if usable(ec) else np.finfo(np.float64).max
        step_norm = float(np.sqrt(sum((x[i] - cand[i]) ** 2 for i in range(7))))
        if step_norm <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            term, why = CONVERGENCE, "parameter_tolerance"; break
        cost_change = x_cost - cand_cost
        it_dc[it] = cost_change
        if abs(cost_change) <= o["function_tolerance"] * x_cost:
            term, why = CONVERGENCE, "function_tolerance"; break
        rel = cost_change / model_cost_change
        if rel > o["min_relative_decrease"]:
            x = cand
            x_norm = x_norm_of(x, held)
            x_cost = ec["cost"]
            JtJ, Jtr = np.asarray(ec["JtJ"]), np.asarray(ec["Jtr"])
            A, g = scale(JtJ, Jtr)
            it_g[it] = grad_max(x, Jtr); it_cost[it] = x_cost; it_ok[it] = 1
            s["num_successful_steps"] += 1
            f = 2.0 * rel - 1.0
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - f * f * f))
            decrease_factor, reuse_diagonal = 2.0, False
        else:
            s["num_unsuccessful_steps"] += 1
            radius = radius / decrease_factor
            decrease_factor *= 2.0
            reuse_diagonal = True
        it_radius[it] = radius
    s.update(termination=term, why=why, num_iterations=it, final_cost=x_cost, it_cost=it_cost, it_radius=it_radius,
             it_successful=it_ok, it_gradient_max_norm=it_g, it_cost_change=it_dc, final_Jtr=np.array(Jtr))
    return x[:4].copy(), x[4:].copy(), s
