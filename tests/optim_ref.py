"""A float64 numpy restatement of the reference's update -- clip_grad_norm_(max_norm) over all gradients, then
torch.optim.AdamW(amsgrad) with decoupled weight decay -- the seeded parameter set the optimiser tests share, the
torch composition they compare with, and the bars.

    total_norm = sqrt(sum g^2)       coef = min(1, max_norm / (total_norm + 1e-6))       g' = g coef
    p *= 1 - lr wd      m += (g' - m)(1 - b1)      v = v b2 + (1 - b2) g'^2      vmax = max(vmax, v)
    p -= lr / (1 - b1^t) * m / (sqrt(vmax) / sqrt(1 - b2^t) + eps)             (v for vmax without amsgrad)

``mutate`` plants one of five textbook mistakes; tests/test_optim_ref.py shows that the bars catch each of them.
"""
import numpy as np

SIZES = [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 12289, 131072]
GSCALES = (1e-4, 1e-2, 1.0)        # at max_norm 0.5 the first is never clipped, the others always
STEPS = 5
LRS = (2e-4, 6e-4, 1e-3, 1e-3, 5e-4)          # warm-up, plateau, a StepLR drop
MAX_NORM = 0.5
MUTATIONS = ("no_running_max", "no_bias_correction", "l2_decay", "eps_inside_sqrt", "unclamped_clip")

# the bars of tests/test_gpu_optim.py (tests/test_optim_ref.py holds torch's own float32 to half of each)
BAR_DP = 1e-4          # p_T - p_0: conftest.assert_parity's default, normwise and element-wise
BAR_STATE = 1e-5       # exp_avg, exp_avg_sq, max_exp_avg_sq: normwise and element-wise
BAR_NORM = 5e-6        # total_norm: relative


class Case:
    """the test parameter set: SIZES, one 2-D tensor, one empty tensor and one 257-element tensor (which the GPU test
    places on a 4-byte-misaligned address); values normal * sqrt(2 / 256); gradients normal * gscale * (1 + t) with
    every 7th element scaled by 1e-3; the parameter ``absent`` has no gradient on step 2"""

    def __init__(self, gscale, seed=0):
        rng = np.random.default_rng(1234 + seed)
        self.shapes = [(n,) for n in SIZES] + [(33, 65), (0,), (257,)]
        self.misaligned = len(self.shapes) - 1
        self.absent = SIZES.index(4097)
        self.params = [(rng.standard_normal(s) * np.sqrt(2.0 / 256)).astype(np.float32) for s in self.shapes]
        self.grads = []
        for t in range(STEPS):
            step = []
            for i, s in enumerate(self.shapes):
                g = rng.standard_normal(s) * gscale * (1 + t)
                g.reshape(-1)[::7] *= 1e-3
                step.append(None if (t == 2 and i == self.absent) else g.astype(np.float32))
            self.grads.append(step)


def total_norm(grads):
    return float(np.sqrt(sum(float(np.sum(np.square(g.astype(np.float64)))) for g in grads if g is not None)))


def run(case, amsgrad=True, max_norm=MAX_NORM, lrs=LRS, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, mutate=None,
        steps=STEPS, state=None):
    """float64.  Returns dict(p, exp_avg, exp_avg_sq, max_exp_avg_sq (lists of arrays), step (list), norms (per step,
    before the clip)).  ``state``: continue from an earlier result."""
    assert mutate is None or mutate in MUTATIONS
    b1, b2 = betas
    if state is None:
        p = [a.astype(np.float64) for a in case.params]
        m = [np.zeros_like(a) for a in p]
        v = [np.zeros_like(a) for a in p]
        vmax = [np.zeros_like(a) for a in p]
        count = [0] * len(p)
        norms = []
        first = 0
    else:
        p, m, v, vmax = ([a.copy() for a in state[k]] for k in ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
        count, norms, first = list(state["step"]), list(state["norms"]), len(state["norms"])
    for t in range(first, first + steps):
        grads = case.grads[t]
        lr = lrs[t]
        coef = 1.0
        if max_norm is not None:
            norms.append(total_norm(grads))
            coef = max_norm / (norms[-1] + 1e-6)
            if mutate != "unclamped_clip":
                coef = min(1.0, coef)
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.astype(np.float64) * coef
            count[i] += 1
            if mutate == "l2_decay":
                g = g + weight_decay * p[i]
            else:
                p[i] *= 1.0 - lr * weight_decay
            m[i] += (g - m[i]) * (1.0 - b1)
            v[i] = v[i] * b2 + (1.0 - b2) * g * g
            vmax[i] = v[i].copy() if mutate == "no_running_max" else np.maximum(vmax[i], v[i])
            top = vmax[i] if amsgrad else v[i]
            bc1 = 1.0 - b1 ** count[i]
            bc2 = 1.0 - b2 ** count[i]
            if mutate == "no_bias_correction":
                bc1 = bc2 = 1.0
            if mutate == "eps_inside_sqrt":
                denom = np.sqrt(top / bc2 + eps)
            else:
                denom = np.sqrt(top) / np.sqrt(bc2) + eps
            p[i] -= lr / bc1 * m[i] / denom
    return dict(p=p, exp_avg=m, exp_avg_sq=v, max_exp_avg_sq=vmax, step=count, norms=norms)


def torch_run(case, dtype, device="cpu", amsgrad=True, max_norm=MAX_NORM, lrs=LRS, weight_decay=0.01, steps=STEPS,
              make_params=None):
    """the reference's composition: clip_grad_norm_ + torch.optim.AdamW, in ``dtype`` on ``device``; same result
    layout as ``run`` (numpy float64 arrays).  Parameters and gradients are copies: the case is never written."""
    import torch
    if make_params is None:
        params = [torch.nn.Parameter(torch.tensor(a, device=device, dtype=dtype)) for a in case.params]
    else:
        params = make_params()
    opt = torch.optim.AdamW(params, lr=lrs[0], betas=(0.9, 0.999), eps=1e-8, amsgrad=amsgrad,
                            weight_decay=weight_decay)
    norms = []
    for t in range(steps):
        for pg in opt.param_groups:
            pg["lr"] = lrs[t]
        for q, g in zip(params, case.grads[t]):
            q.grad = None if g is None else torch.tensor(g, device=device, dtype=dtype)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
    return torch_result(opt, params, norms)


def torch_result(opt, params, norms=()):
    def field(q, key):
        st = opt.state.get(q, {})
        if key not in st:
            return np.zeros(tuple(q.shape))
        return st[key].detach().double().cpu().numpy()
    return dict(p=[q.detach().double().cpu().numpy() for q in params],
                exp_avg=[field(q, "exp_avg") for q in params], exp_avg_sq=[field(q, "exp_avg_sq") for q in params],
                max_exp_avg_sq=[field(q, "max_exp_avg_sq") for q in params],
                step=[int(opt.state[q]["step"]) if q in opt.state and "step" in opt.state[q] else 0 for q in params],
                norms=list(norms))


def errors(got, ref, case, amsgrad=True):
    """the worst figures of ``got`` against ``ref`` over all tensors, in the measures of the bars: dict(dp_norm,
    dp_elem, state, norm)"""
    import conftest
    out = dict(dp_norm=0.0, dp_elem=0.0, state=0.0, norm=0.0)
    for i, p0 in enumerate(case.params):
        if p0.size == 0:
            continue
        p0 = p0.astype(np.float64)
        a, b = got["p"][i] - p0, ref["p"][i] - p0
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            return dict(dp_norm=np.inf, dp_elem=np.inf, state=np.inf, norm=np.inf)
        out["dp_norm"] = max(out["dp_norm"], conftest.rel_err(a, b))
        out["dp_elem"] = max(out["dp_elem"], conftest.elem_err(a, b))
        for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ()):
            out["state"] = max(out["state"], conftest.rel_err(got[k][i], ref[k][i]),
                               conftest.elem_err(got[k][i], ref[k][i]))
    for a, b in zip(got["norms"], ref["norms"]):
        out["norm"] = max(out["norm"], abs(a - b) / b)
    return out


def within_bars(err, scale=1.0):
    return (err["dp_norm"] <= scale * BAR_DP and err["dp_elem"] <= scale * BAR_DP
            and err["state"] <= scale * BAR_STATE and err["norm"] <= scale * BAR_NORM)
