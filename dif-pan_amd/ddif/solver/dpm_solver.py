"""Drop-in for the part of the reference `solver/dpm_solver.py` (vendored DPM-Solver v2) that the DDIF hot path
reaches: `NoiseScheduleVP('discrete')` (:6-175), `model_wrapper` (:178-342) and `DPM_Solver` (:345-962, 1020-1253) with
`sample(method="multistep" | "singlestep" | "singlestep_fixed")`, both solver types and both algorithm types.

Scalar schedule math stays on the host as fp32 torch scalars (the reference evaluates the same expressions as 0-d /
1-element fp32 tensors); the tensor work of a whole sampling run -- every network evaluation, the x_start<->eps
round trip, the corrector (the image-space clamp or dynamic thresholding, whose per-sample quantile is a selection
kernel in front of the data prediction) and the multistep updates -- is ONE call into libddif (`ddif_plan_sample_dpmpp`)
when the model is a ddif `UNetSR3`.  Singlestep runs, solver_type="taylor", algorithm_type="dpmsolver", denoise_to_zero
and return_intermediate are ONE call too (`ddif_plan_sample_dpm`) on a solver program built here: a flat op list over a few
state and model registers, every scalar the reference's own fp32 expression (`_build_program`).  Classifier-free guidance
(`model_wrapper(guidance_scale != 1, unconditional_condition=...)`, reference :330-338) runs the same programs, for every method, through
`ddif_plan_sample_dpm_guided` on a plan of batch 2B whose cond is `cat([unconditional_condition, condition])`: the network sees the doubled batch
once per evaluation and the launch behind it combines eps_u + scale * (eps_c - eps_u) before the corrector and the update.  The reference itself
runs its guided branch with model_type="noise" and B = 1 only (with "x_start" / "v" its (2,)-shaped alpha_t does not broadcast against the doubled
batch; B > 1 fails the same way everywhere in its solver); here every model type and any B run.  guidance_scale == 1 or no unconditional_condition
is the single conditional evaluation as before.  Any other model / corrector
takes the generic loops below (same algorithm, model called per evaluation through the reference's update methods; dynamic
thresholding there is the stateless `ddif_dynamic_threshold`).  Out of scope and rejected loudly: continuous schedules, the
adaptive solver (its step size depends on a norm read back from the device every step), classifier guidance (SURVEY.md
section 2, row 3).
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional

import torch

from ..runtime import DdifError


def interpolate_fn(x: torch.Tensor, xp: torch.Tensor, yp: torch.Tensor) -> torch.Tensor:
    """Piecewise-linear y(x) through the keypoints (xp, yp) with linear extrapolation beyond both ends
    (reference :1261-1300).  x: [N, C], xp / yp: [C, K] -> [N, C].  A query equal to a keypoint takes the segment
    on its LEFT (the reference sorts the query in front of the equal keypoint)."""
    N, K = x.shape[0], xp.shape[1]
    out = torch.empty_like(x)
    for c in range(x.shape[1]):
        xs, ys = xp[c], yp[c]
        below = (xs.unsqueeze(0) < x[:, c].unsqueeze(1)).sum(dim=1)  # keypoints strictly below each query
        lo = torch.where(below == 0, torch.zeros_like(below), torch.where(below == K, torch.full_like(below, K - 2), below - 1))
        x0, x1, y0, y1 = xs[lo], xs[lo + 1], ys[lo], ys[lo + 1]
        out[:, c] = y0 + (x[:, c] - x0) * (y1 - y0) / (x1 - x0)
    return out


class NoiseScheduleVP:
    def __init__(self, schedule="discrete", betas=None, alphas_cumprod=None, continuous_beta_0=0.1,
                 continuous_beta_1=20.0, dtype=torch.float32):
        if schedule != "discrete":
            raise DdifError(f"NoiseScheduleVP(schedule='{schedule}'): only 'discrete' is in scope of the HIP path")
        self.schedule = schedule
        if betas is not None:
            log_alphas = 0.5 * torch.log(1 - betas.detach().cpu()).cumsum(dim=0)
        else:
            assert alphas_cumprod is not None
            log_alphas = 0.5 * torch.log(alphas_cumprod.detach().cpu())
        self.total_N = len(log_alphas)
        self.T = 1.0
        self.t_array = torch.linspace(0.0, 1.0, self.total_N + 1)[1:].reshape((1, -1)).to(dtype=dtype)
        self.log_alpha_array = log_alphas.reshape((1, -1)).to(dtype=dtype)

    def marginal_log_mean_coeff(self, t):
        t = t.detach().cpu()
        return interpolate_fn(t.reshape((-1, 1)), self.t_array, self.log_alpha_array).reshape((-1))

    def marginal_alpha(self, t):
        return torch.exp(self.marginal_log_mean_coeff(t))

    def marginal_std(self, t):
        return torch.sqrt(1.0 - torch.exp(2.0 * self.marginal_log_mean_coeff(t)))

    def marginal_lambda(self, t):
        la = self.marginal_log_mean_coeff(t)
        return la - 0.5 * torch.log(1.0 - torch.exp(2.0 * la))

    def inverse_lambda(self, lamb):
        lamb = lamb.detach().cpu()
        log_alpha = -0.5 * torch.logaddexp(torch.zeros((1,)), -2.0 * lamb)
        t = interpolate_fn(log_alpha.reshape((-1, 1)), torch.flip(self.log_alpha_array, [1]), torch.flip(self.t_array, [1]))
        return t.reshape((-1,))


class ImageSpaceClamp:
    """The x0 corrector the engine uses: clamp in image space around the up-sampled LMS,
    x0 <- clamp(x0 + lms, lo, hi) - lms  (reference diffusion_engine.py:43-49).  A recognisable object (rather than
    an opaque closure) so `DPM_Solver` can run it inside the fused kernels."""

    def __init__(self, lms: torch.Tensor, lo: float = 0.0, hi: float = 1.0):
        self.lms, self.lo, self.hi = lms, float(lo), float(hi)

    def __call__(self, x0, t=None):
        return (x0 + self.lms).clamp(self.lo, self.hi) - self.lms


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond", condition=None,
                  unconditional_condition=None, guidance_scale=1.0, classifier_fn=None, classifier_kwargs={}):
    """Reference :178-342.  Returns model_fn(x, t_continuous) -> predicted noise."""
    assert model_type in ["noise", "x_start", "v", "score"]
    assert guidance_type in ["uncond", "classifier", "classifier-free"]
    if guidance_type == "classifier":
        raise DdifError("classifier guidance is out of scope of the HIP path")
    guided = guidance_type == "classifier-free" and not (guidance_scale == 1.0 or unconditional_condition is None)  # (:331)
    if guided:
        if not math.isfinite(float(guidance_scale)):
            raise DdifError(f"model_wrapper: guidance_scale {guidance_scale!r} is not finite")
        if not (torch.is_tensor(condition) and torch.is_tensor(unconditional_condition)):
            raise DdifError("model_wrapper: classifier-free guidance needs `condition` and `unconditional_condition` tensors")
        u, c = unconditional_condition, condition
        if u.shape != c.shape or u.dtype != c.dtype or u.device != c.device:
            raise DdifError(f"model_wrapper: unconditional_condition ({tuple(u.shape)}, {u.dtype}, {u.device}) does not match condition "
                            f"({tuple(c.shape)}, {c.dtype}, {c.device}): the network runs once on cat([unconditional_condition, condition])")

    def get_model_input_time(t_continuous):
        return (t_continuous - 1.0 / noise_schedule.total_N) * 1000.0  # float model time (:285-286)

    def bshape(v, x):
        return v.to(x.device).reshape((-1,) + (1,) * (x.dim() - 1))  # broadcasts for any B (the reference: B==1 only)

    def noise_pred_fn(x, t_continuous, cond=None):
        t_input = get_model_input_time(t_continuous)
        out = model(x, t_input, **model_kwargs) if cond is None else model(x, t_input, cond, **model_kwargs)
        if model_type == "noise":
            return out
        a, s = noise_schedule.marginal_alpha(t_continuous), noise_schedule.marginal_std(t_continuous)
        if model_type == "x_start":
            return (x - bshape(a, x) * out) / bshape(s, x)
        if model_type == "v":
            return bshape(a, x) * out + bshape(s, x) * x
        return -bshape(s, x) * out

    def model_fn(x, t_continuous):
        if not guided:
            return noise_pred_fn(x, t_continuous, cond=condition if guidance_type == "classifier-free" else None)
        x_in = torch.cat([x] * 2)  # one network call on [unconditional; conditional] (:334-338)
        t_in = torch.cat([t_continuous] * 2)
        c_in = torch.cat([unconditional_condition, condition])
        noise_uncond, noise = noise_pred_fn(x_in, t_in, cond=c_in).chunk(2)
        return noise_uncond + guidance_scale * (noise - noise_uncond)

    model_fn.ddif = dict(model=model, noise_schedule=noise_schedule, model_type=model_type, model_kwargs=model_kwargs,
                         guidance_type=guidance_type, condition=condition, guidance_scale=guidance_scale, unconditional_condition=unconditional_condition)
    return model_fn


class DPM_Solver:
    def __init__(self, model_fn, noise_schedule, algorithm_type="dpmsolver++", correcting_x0_fn=None,
                 correcting_xt_fn=None, thresholding_max_val=1.0, dynamic_thresholding_ratio=0.995):
        assert algorithm_type in ["dpmsolver", "dpmsolver++"]
        self._model_fn = model_fn
        self.model = lambda x, t: model_fn(x, t.expand((x.shape[0])))
        self.noise_schedule = noise_schedule
        self.algorithm_type = algorithm_type
        self.correcting_x0_fn = self.dynamic_thresholding_fn if correcting_x0_fn == "dynamic_thresholding" else correcting_x0_fn  # reference :417-420
        self.correcting_xt_fn = correcting_xt_fn
        self.dynamic_thresholding_ratio = dynamic_thresholding_ratio
        self.thresholding_max_val = thresholding_max_val

    # ---- reference helpers kept for API compatibility ---------------------------------------------------------------
    def dynamic_thresholding_fn(self, x0, t=None):
        """Reference :424-433 on device tensors: s = max(quantile(|x0_b|, dynamic_thresholding_ratio), thresholding_max_val) per sample, then
        clamp(x0, -s, s) / s.  One selection kernel + one elementwise kernel of libddif."""
        from ..runtime import dynamic_threshold

        return dynamic_threshold(x0, float(self.dynamic_thresholding_ratio), float(self.thresholding_max_val), symmetric=True)[0]

    def noise_prediction_fn(self, x, t):
        return self.model(x, t)

    def data_prediction_fn(self, x, t):
        noise = self.noise_prediction_fn(x, t)
        a, s = self.noise_schedule.marginal_alpha(t), self.noise_schedule.marginal_std(t)
        a, s = a.to(x.device).reshape(-1, *([1] * (x.dim() - 1))), s.to(x.device).reshape(-1, *([1] * (x.dim() - 1)))
        x0 = (x - s * noise) / a
        if self.correcting_x0_fn is not None:
            x0 = self.correcting_x0_fn(x0, t)
        return x0

    def model_fn(self, x, t):
        return self.data_prediction_fn(x, t) if self.algorithm_type == "dpmsolver++" else self.noise_prediction_fn(x, t)

    def get_time_steps(self, skip_type, t_T, t_0, N, device=None):
        if skip_type == "logSNR":
            lt = self.noise_schedule.marginal_lambda(torch.tensor(t_T))
            l0 = self.noise_schedule.marginal_lambda(torch.tensor(t_0))
            return self.noise_schedule.inverse_lambda(torch.linspace(lt.item(), l0.item(), N + 1))
        if skip_type == "time_uniform":
            return torch.linspace(t_T, t_0, N + 1)
        if skip_type == "time_quadratic":
            return torch.linspace(t_T ** 0.5, t_0 ** 0.5, N + 1).pow(2)
        raise ValueError(f"Unsupported skip_type {skip_type}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'")

    # ---- per-update scalars (reference :555-588, 804-845, 862-912), fp32 like the reference ----------------------------
    def _update_coefs(self, tprev: List[torch.Tensor], t: torch.Tensor, order: int) -> dict:
        ns = self.noise_schedule
        lam_t, lam_0 = ns.marginal_lambda(t), ns.marginal_lambda(tprev[-1])
        h = lam_t - lam_0
        a_t = torch.exp(ns.marginal_log_mean_coeff(t))
        s_t, s_0 = ns.marginal_std(t), ns.marginal_std(tprev[-1])
        pp = self.algorithm_type == "dpmsolver++"
        phi1 = torch.expm1(-h) if pp else torch.expm1(h)
        if pp:
            c = dict(cx=float(s_t / s_0), a_phi1=float(a_t * phi1))
        else:  # noise prediction (:590-596, 846-853, 902-911): the same update expressions over another coefficient family
            c = dict(cx=float(torch.exp(ns.marginal_log_mean_coeff(t) - ns.marginal_log_mean_coeff(tprev[-1]))), a_phi1=float(s_t * phi1))
        c.update(inv_r0=0.0, inv_r1=0.0, r0_frac=0.0, inv_r01=0.0, a_phi2=0.0, a_phi3=0.0)
        if order >= 2:
            h0 = lam_0 - ns.marginal_lambda(tprev[-2])
            r0 = h0 / h
            c["inv_r0"] = float(1.0 / r0)
            # solver_type="taylor", order 2 (:841-845, 855-859): x_t = cx*x - a_phi1*m0 + tay2 * D1_0
            c["tay2"] = float(a_t * (phi1 / h + 1.0)) if pp else -float(s_t * (phi1 / h - 1.0))
        if order == 3:
            h1 = ns.marginal_lambda(tprev[-2]) - ns.marginal_lambda(tprev[-3])
            r1 = h1 / h
            phi2 = phi1 / h + 1.0 if pp else phi1 / h - 1.0
            phi3 = phi2 / h - 0.5
            c.update(inv_r1=float(1.0 / r1), r0_frac=float(r0 / (r0 + r1)), inv_r01=float(1.0 / (r0 + r1)))
            if pp:
                c.update(a_phi2=float(a_t * phi2), a_phi3=float(a_t * phi3))
            else:  # - (sigma_t * phi_2) * D1: the minus goes into the scalar
                c.update(a_phi2=-float(s_t * phi2), a_phi3=float(s_t * phi3))
        return c

    @staticmethod
    def _apply_update(x, models, c, order, taylor=False):
        m0 = models[-1]
        v = c["cx"] * x - c["a_phi1"] * m0
        if order == 2 and taylor:
            v = v + c["tay2"] * (c["inv_r0"] * (m0 - models[-2]))
        elif order == 2:
            d1 = c["inv_r0"] * (m0 - models[-2])
            v = v - (0.5 * c["a_phi1"]) * d1
        elif order == 3:
            d10 = c["inv_r0"] * (m0 - models[-2])
            d11 = c["inv_r1"] * (models[-2] - models[-3])
            d1 = d10 + c["r0_frac"] * (d10 - d11)
            d2 = c["inv_r01"] * (d10 - d11)
            v = (v + c["a_phi2"] * d1) - c["a_phi3"] * d2
        return v

    def _fused_target(self):
        """(UNetSR3, cond, clamp) when the whole run can execute inside libddif, else None.  clamp: None, (lo, hi) of an ImageSpaceClamp, or the
        string "dynamic" for this solver's own dynamic_thresholding_fn (the plan's threshold mode "solver")."""
        meta = getattr(self._model_fn, "ddif", None)
        if meta is None or self.correcting_xt_fn is not None:  # (under algorithm_type="dpmsolver" the corrector reaches the library for the final denoise only)
            return None
        from ..models.sr3_dwt import UNetSR3

        if not isinstance(meta["model"], UNetSR3) or meta["model_type"] not in ("x_start", "noise", "v") or meta["model_kwargs"]:
            return None
        if meta["guidance_type"] != "classifier-free" or meta["condition"] is None:
            return None
        cx0 = self.correcting_x0_fn
        if cx0 is None:
            return meta["model"], meta["condition"], None
        if getattr(cx0, "__func__", None) is DPM_Solver.dynamic_thresholding_fn and getattr(cx0, "__self__", None) is self:
            return meta["model"], meta["condition"], "dynamic"
        if isinstance(cx0, ImageSpaceClamp):
            cond, C = meta["condition"], meta["model"].cfg["out_channel"]
            if cx0.lms.shape == cond[:, :C].shape and cx0.lms.data_ptr() == cond[:, :C].data_ptr() or \
                    torch.equal(cx0.lms, cond[:, :C]):
                return meta["model"], cond, (cx0.lo, cx0.hi)
        return None

    def _guidance(self):
        """(guidance_scale, unconditional_condition) when model_wrapper takes its guided branch (reference :333-338), else None (:331-332)."""
        meta = getattr(self._model_fn, "ddif", None)
        if meta is None or meta["guidance_type"] != "classifier-free":
            return None
        scale, uncond = meta.get("guidance_scale", 1.0), meta.get("unconditional_condition")
        return None if (scale == 1.0 or uncond is None) else (float(scale), uncond)

    # ---- singlestep scalars (reference :555-600, 602-802), fp32 1-element tensors / Python floats exactly as the reference forms them ---------------
    def _first_coefs(self, s, t):
        """(c0, c1) of x_t = c0 * x - c1 * model_s (:577-600)."""
        ns = self.noise_schedule
        h = ns.marginal_lambda(t) - ns.marginal_lambda(s)
        if self.algorithm_type == "dpmsolver++":
            return float(ns.marginal_std(t) / ns.marginal_std(s)), float(torch.exp(ns.marginal_log_mean_coeff(t)) * torch.expm1(-h))
        return float(torch.exp(ns.marginal_log_mean_coeff(t) - ns.marginal_log_mean_coeff(s))), float(ns.marginal_std(t) * torch.expm1(h))

    def _second_coefs(self, s, t, r1, solver_type):
        """s1 and the scalars of x_s1 = c0*x - c1*m_s and x_t = (c0*x - c1*m_s) + c2*(m_s1 - m_s) (:619-677)."""
        if solver_type not in ["dpmsolver", "taylor"]:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        if r1 is None:
            r1 = 0.5
        ns = self.noise_schedule
        lambda_s, lambda_t = ns.marginal_lambda(s), ns.marginal_lambda(t)
        h = lambda_t - lambda_s
        s1 = ns.inverse_lambda(lambda_s + r1 * h)
        log_alpha_s, log_alpha_s1, log_alpha_t = ns.marginal_log_mean_coeff(s), ns.marginal_log_mean_coeff(s1), ns.marginal_log_mean_coeff(t)
        sigma_s, sigma_s1, sigma_t = ns.marginal_std(s), ns.marginal_std(s1), ns.marginal_std(t)
        alpha_s1, alpha_t = torch.exp(log_alpha_s1), torch.exp(log_alpha_t)
        if self.algorithm_type == "dpmsolver++":
            phi_11, phi_1 = torch.expm1(-r1 * h), torch.expm1(-h)
            xs1 = (sigma_s1 / sigma_s, alpha_s1 * phi_11)
            c2 = -((0.5 / r1) * (alpha_t * phi_1)) if solver_type == "dpmsolver" else (1. / r1) * (alpha_t * (phi_1 / h + 1.))
            xt = (sigma_t / sigma_s, alpha_t * phi_1, c2)
        else:
            phi_11, phi_1 = torch.expm1(r1 * h), torch.expm1(h)
            xs1 = (torch.exp(log_alpha_s1 - log_alpha_s), sigma_s1 * phi_11)
            c2 = -((0.5 / r1) * (sigma_t * phi_1)) if solver_type == "dpmsolver" else -((1. / r1) * (sigma_t * (phi_1 / h - 1.)))
            xt = (torch.exp(log_alpha_t - log_alpha_s), sigma_t * phi_1, c2)
        return dict(s1=s1, xs1=tuple(float(v) for v in xs1), xt=tuple(float(v) for v in xt))

    def _third_coefs(self, s, t, r1, r2, solver_type):
        """s1, s2 and the scalars of x_s1, x_s2 and x_t (:703-797).  xt: 3 scalars (lin2 over m_s2 - m_s) or the 9 of tay3 (csrc/kernels_misc.h)."""
        if solver_type not in ["dpmsolver", "taylor"]:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        if r1 is None:
            r1 = 1. / 3.
        if r2 is None:
            r2 = 2. / 3.
        ns = self.noise_schedule
        lambda_s, lambda_t = ns.marginal_lambda(s), ns.marginal_lambda(t)
        h = lambda_t - lambda_s
        s1 = ns.inverse_lambda(lambda_s + r1 * h)
        s2 = ns.inverse_lambda(lambda_s + r2 * h)
        log_alpha_s, log_alpha_s1, log_alpha_s2, log_alpha_t = (ns.marginal_log_mean_coeff(s), ns.marginal_log_mean_coeff(s1), ns.marginal_log_mean_coeff(s2),
                                                                ns.marginal_log_mean_coeff(t))
        sigma_s, sigma_s1, sigma_s2, sigma_t = ns.marginal_std(s), ns.marginal_std(s1), ns.marginal_std(s2), ns.marginal_std(t)
        alpha_s1, alpha_s2, alpha_t = torch.exp(log_alpha_s1), torch.exp(log_alpha_s2), torch.exp(log_alpha_t)
        if self.algorithm_type == "dpmsolver++":
            phi_11, phi_12, phi_1 = torch.expm1(-r1 * h), torch.expm1(-r2 * h), torch.expm1(-h)
            phi_22 = torch.expm1(-r2 * h) / (r2 * h) + 1.
            phi_2 = phi_1 / h + 1.
            phi_3 = phi_2 / h - 0.5
            xs1 = (sigma_s1 / sigma_s, alpha_s1 * phi_11)
            xs2 = (sigma_s2 / sigma_s, alpha_s2 * phi_12, r2 / r1 * (alpha_s2 * phi_22))
            base = (sigma_t / sigma_s, alpha_t * phi_1)
            if solver_type == "dpmsolver":
                xt = base + ((1. / r2) * (alpha_t * phi_2),)
            else:
                xt = base + (alpha_t * phi_2, 1. / r1, 1. / r2, r1, r2, r2 - r1, alpha_t * phi_3)
        else:
            phi_11, phi_12, phi_1 = torch.expm1(r1 * h), torch.expm1(r2 * h), torch.expm1(h)
            phi_22 = torch.expm1(r2 * h) / (r2 * h) - 1.
            phi_2 = phi_1 / h - 1.
            phi_3 = phi_2 / h - 0.5
            xs1 = (torch.exp(log_alpha_s1 - log_alpha_s), sigma_s1 * phi_11)
            xs2 = (torch.exp(log_alpha_s2 - log_alpha_s), sigma_s2 * phi_12, -(r2 / r1 * (sigma_s2 * phi_22)))
            base = (torch.exp(log_alpha_t - log_alpha_s), sigma_t * phi_1)
            if solver_type == "dpmsolver":
                xt = base + (-((1. / r2) * (sigma_t * phi_2)),)
            else:
                xt = base + (-(sigma_t * phi_2), 1. / r1, 1. / r2, r1, r2, r2 - r1, sigma_t * phi_3)
        f = lambda tup: tuple(float(v) for v in tup)
        return dict(s1=s1, s2=s2, xs1=f(xs1), xs2=f(xs2), xt=f(xt))

    @staticmethod
    def _lin2(x, m0, c, ma=None, mb=None):
        v = c[0] * x - c[1] * m0
        return v if ma is None else v + c[2] * (ma - mb)

    @staticmethod
    def _tay3(x, m0, m1, m2, c):
        """c = (c0, c1, a_phi2, 1/r1, 1/r2, r1, r2, r2 - r1, a_phi3) (:749-758, 788-797)."""
        D1_0 = c[3] * (m1 - m0)
        D1_1 = c[4] * (m2 - m0)
        D1 = (c[6] * D1_0 - c[5] * D1_1) / c[7]
        D2 = 2. * (D1_1 - D1_0) / c[7]
        return ((c[0] * x - c[1] * m0) + c[2] * D1) - c[8] * D2

    # ---- the reference's update methods (signatures and defaults of :490-1053); they carry the generic path --------------------------------------
    def get_orders_and_timesteps_for_singlestep_solver(self, steps, order, skip_type, t_T, t_0, device=None):
        if order == 3:
            K = steps // 3 + 1
            if steps % 3 == 0:
                orders = [3, ] * (K - 2) + [2, 1]
            elif steps % 3 == 1:
                orders = [3, ] * (K - 1) + [1]
            else:
                orders = [3, ] * (K - 1) + [2]
        elif order == 2:
            if steps % 2 == 0:
                K = steps // 2
                orders = [2, ] * K
            else:
                K = steps // 2 + 1
                orders = [2, ] * (K - 1) + [1]
        elif order == 1:
            K = 1
            orders = [1, ] * steps
        else:
            raise ValueError("'order' must be '1' or '2' or '3'.")
        if skip_type == "logSNR":
            timesteps_outer = self.get_time_steps(skip_type, t_T, t_0, K, device)  # (order 1: K = 1 -- two times for `steps` updates, as in the reference)
        else:
            timesteps_outer = self.get_time_steps(skip_type, t_T, t_0, steps, device)[torch.cumsum(torch.tensor([0, ] + orders), 0)]
        return timesteps_outer, orders

    def denoise_to_zero_fn(self, x, s):
        return self.data_prediction_fn(x, s)

    def dpm_solver_first_update(self, x, s, t, model_s=None, return_intermediate=False):
        c = self._first_coefs(s, t)
        if model_s is None:
            model_s = self.model_fn(x, s)
        x_t = self._lin2(x, model_s, c)
        return (x_t, {"model_s": model_s}) if return_intermediate else x_t

    def singlestep_dpm_solver_second_update(self, x, s, t, r1=0.5, model_s=None, return_intermediate=False, solver_type="dpmsolver"):
        c = self._second_coefs(s, t, r1, solver_type)
        if model_s is None:
            model_s = self.model_fn(x, s)
        x_s1 = self._lin2(x, model_s, c["xs1"])
        model_s1 = self.model_fn(x_s1, c["s1"])
        x_t = self._lin2(x, model_s, c["xt"], model_s1, model_s)
        return (x_t, {"model_s": model_s, "model_s1": model_s1}) if return_intermediate else x_t

    def singlestep_dpm_solver_third_update(self, x, s, t, r1=1. / 3., r2=2. / 3., model_s=None, model_s1=None, return_intermediate=False, solver_type="dpmsolver"):
        c = self._third_coefs(s, t, r1, r2, solver_type)
        if model_s is None:
            model_s = self.model_fn(x, s)
        if model_s1 is None:
            x_s1 = self._lin2(x, model_s, c["xs1"])
            model_s1 = self.model_fn(x_s1, c["s1"])
        x_s2 = self._lin2(x, model_s, c["xs2"], model_s1, model_s)
        model_s2 = self.model_fn(x_s2, c["s2"])
        if solver_type == "dpmsolver":
            x_t = self._lin2(x, model_s, c["xt"], model_s2, model_s)
        else:
            x_t = self._tay3(x, model_s, model_s1, model_s2, c["xt"])
        return (x_t, {"model_s": model_s, "model_s1": model_s1, "model_s2": model_s2}) if return_intermediate else x_t

    def multistep_dpm_solver_second_update(self, x, model_prev_list, t_prev_list, t, solver_type="dpmsolver"):
        if solver_type not in ["dpmsolver", "taylor"]:
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        c = self._update_coefs([tp.reshape(1) for tp in t_prev_list[-2:]], t.reshape(1), 2)
        return self._apply_update(x, list(model_prev_list[-2:]), c, 2, taylor=solver_type == "taylor")

    def multistep_dpm_solver_third_update(self, x, model_prev_list, t_prev_list, t, solver_type="dpmsolver"):
        model_prev_2, model_prev_1, model_prev_0 = model_prev_list
        t_prev_2, t_prev_1, t_prev_0 = t_prev_list
        c = self._update_coefs([t_prev_2.reshape(1), t_prev_1.reshape(1), t_prev_0.reshape(1)], t.reshape(1), 3)
        return self._apply_update(x, [model_prev_2, model_prev_1, model_prev_0], c, 3)

    def singlestep_dpm_solver_update(self, x, s, t, order, return_intermediate=False, solver_type="dpmsolver", r1=None, r2=None):
        if order == 1:
            return self.dpm_solver_first_update(x, s, t, return_intermediate=return_intermediate)
        elif order == 2:
            return self.singlestep_dpm_solver_second_update(x, s, t, return_intermediate=return_intermediate, solver_type=solver_type, r1=r1)
        elif order == 3:
            return self.singlestep_dpm_solver_third_update(x, s, t, return_intermediate=return_intermediate, solver_type=solver_type, r1=r1, r2=r2)
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    def multistep_dpm_solver_update(self, x, model_prev_list, t_prev_list, t, order, solver_type="dpmsolver"):
        if order == 1:
            return self.dpm_solver_first_update(x, t_prev_list[-1], t, model_s=model_prev_list[-1])
        elif order == 2:
            return self.multistep_dpm_solver_second_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        elif order == 3:
            return self.multistep_dpm_solver_third_update(x, model_prev_list, t_prev_list, t, solver_type=solver_type)
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))

    def add_noise(self, x, t, noise=None):
        """x_t = alpha_t * x + sigma_t * noise for every time of t: (t_size, batch_size, *shape), squeezed for one time (:1020-1038)."""
        alpha_t, sigma_t = self.noise_schedule.marginal_alpha(t).to(x.device), self.noise_schedule.marginal_std(t).to(x.device)
        if noise is None:
            noise = torch.randn((t.shape[0], *x.shape), device=x.device)
        x = x.reshape((-1, *x.shape))
        shape = (-1,) + (1,) * (x.dim() - 1)
        xt = alpha_t.reshape(shape) * x + sigma_t.reshape(shape) * noise
        return xt.squeeze(0) if t.shape[0] == 1 else xt

    def inverse(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type="time_uniform", method="multistep", lower_order_final=True,
                denoise_to_zero=False, solver_type="dpmsolver", atol=0.0078, rtol=0.05, return_intermediate=False):
        t_0 = 1. / self.noise_schedule.total_N if t_start is None else t_start
        t_T = self.noise_schedule.T if t_end is None else t_end
        assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
        return self.sample(x, steps=steps, t_start=t_0, t_end=t_T, order=order, skip_type=skip_type, method=method, lower_order_final=lower_order_final,
                           denoise_to_zero=denoise_to_zero, solver_type=solver_type, atol=atol, rtol=rtol, return_intermediate=return_intermediate)

    # ---- the schedule of a run: shared by the generic loop and the solver program -------------------------------------------------------------------
    @staticmethod
    def _multistep_orders(steps, order, lower_order_final):
        """Order of the update INTO timesteps[step], step = 1 .. steps (:1193-1210); lower_order_final only with steps < 10."""
        return [step if step < order else (min(order, steps + 1 - step) if lower_order_final and steps < 10 else order) for step in range(1, steps + 1)]

    def _singlestep_schedule(self, steps, order, skip_type, method, t_T, t_0):
        """[(s, t, order, r1, r2)] per outer step (:1223-1235); s, t 0-d fp32 tensors, r1 / r2 0-d fp32 tensors or None."""
        if method == "singlestep":
            timesteps_outer, orders = self.get_orders_and_timesteps_for_singlestep_solver(steps=steps, order=order, skip_type=skip_type, t_T=t_T, t_0=t_0)
        else:
            K = steps // order
            orders = [order, ] * K
            timesteps_outer = self.get_time_steps(skip_type, t_T, t_0, K)
        sched = []
        for step, o in enumerate(orders):
            s, t = timesteps_outer[step], timesteps_outer[step + 1]  # (singlestep, order 1, logSNR: IndexError at step 1, as in the reference)
            timesteps_inner = self.get_time_steps(skip_type, s.item(), t.item(), o)
            lambda_inner = self.noise_schedule.marginal_lambda(timesteps_inner)
            h = lambda_inner[-1] - lambda_inner[0]
            r1 = None if o <= 1 else (lambda_inner[1] - lambda_inner[0]) / h
            r2 = None if o <= 2 else (lambda_inner[2] - lambda_inner[0]) / h
            sched.append((s, t, o, r1, r2))
        return sched

    def _eval_op(self, t, src, dst, kind="eval"):
        ns = self.noise_schedule
        t1 = t.reshape(1)
        return dict(kind=kind, t=t1, t_model=float((t1 - 1.0 / ns.total_N) * 1000.0), alpha=float(ns.marginal_alpha(t1)), sigma=float(ns.marginal_std(t1)), src=src, dst=dst)

    def _build_program(self, steps, order, skip_type, method, lower_order_final, denoise_to_zero, solver_type, return_intermediate, t_T, t_0):
        """The run as a flat op list over state registers (0 x, 1 x_s1, 2 x_s2) and model registers (include/ddif.h ddif_dpm_program).  Every scalar is the
        reference's own fp32 torch expression; `t` of an evaluation (its continuous time, a 1-element fp32 tensor) stays on the op for the tests."""
        ops = []
        emit = (lambda: ops.append(dict(kind="emit", src=0))) if return_intermediate else (lambda: None)
        pad = lambda c: list(c) + [0.0] * (9 - len(c))
        if method == "multistep":
            assert steps >= order
            ts = self.get_time_steps(skip_type, t_T, t_0, steps)
            assert ts.shape[0] - 1 == steps
            ords = self._multistep_orders(steps, order, lower_order_final)
            ops.append(self._eval_op(ts[0], 0, 0))
            emit()  # the initial x (:1190-1191)
            for step in range(1, steps + 1):
                o = ords[step - 1]
                c = self._update_coefs([ts[j].reshape(1) for j in range(step - o, step)], ts[step].reshape(1), o)
                m = [(step - 1 - j) % 3 for j in range(3)]  # newest first
                if o == 2 and solver_type == "taylor":
                    ops.append(dict(kind="update", form="lin2", order=0, src=0, dst=0, m=[m[0], m[0], m[1]], c=pad([c["cx"], c["a_phi1"], c["tay2"], c["inv_r0"]])))
                else:
                    ops.append(dict(kind="update", form="multi", order=o, src=0, dst=0, m=m,
                                    c=pad([c["cx"], c["a_phi1"], c["inv_r0"], c["inv_r1"], c["r0_frac"], c["inv_r01"], c["a_phi2"], c["a_phi3"]])))
                emit()
                if step < steps:  # the final model value is never needed (:1219-1221)
                    ops.append(self._eval_op(ts[step], 0, step % 3))
        else:
            for s, t, o, r1, r2 in self._singlestep_schedule(steps, order, skip_type, method, t_T, t_0):
                ops.append(self._eval_op(s, 0, 0))
                if o == 1:
                    ops.append(dict(kind="update", form="lin1", order=0, src=0, dst=0, m=[0, 0, 0], c=pad(self._first_coefs(s, t))))
                elif o == 2:
                    c = self._second_coefs(s, t, r1, solver_type)
                    ops.append(dict(kind="update", form="lin1", order=0, src=0, dst=1, m=[0, 0, 0], c=pad(c["xs1"])))
                    ops.append(self._eval_op(c["s1"], 1, 1))
                    ops.append(dict(kind="update", form="lin2", order=0, src=0, dst=0, m=[0, 1, 0], c=pad(list(c["xt"]) + [1.0])))
                else:
                    c = self._third_coefs(s, t, r1, r2, solver_type)
                    ops.append(dict(kind="update", form="lin1", order=0, src=0, dst=1, m=[0, 0, 0], c=pad(c["xs1"])))
                    ops.append(self._eval_op(c["s1"], 1, 1))
                    ops.append(dict(kind="update", form="lin2", order=0, src=0, dst=2, m=[0, 1, 0], c=pad(list(c["xs2"]) + [1.0])))
                    ops.append(self._eval_op(c["s2"], 2, 2))
                    if solver_type == "dpmsolver":
                        ops.append(dict(kind="update", form="lin2", order=0, src=0, dst=0, m=[0, 2, 0], c=pad(list(c["xt"]) + [1.0])))
                    else:
                        ops.append(dict(kind="update", form="tay3", order=0, src=0, dst=0, m=[0, 1, 2], c=pad(c["xt"])))
                emit()
        if denoise_to_zero:
            ops.append(self._eval_op(torch.ones((1,)) * t_0, 0, 0, kind="final"))
            emit()
        return ops

    def sample(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type="time_uniform", method="multistep",
               lower_order_final=True, denoise_to_zero=False, solver_type="dpmsolver", atol=0.0078, rtol=0.05,
               return_intermediate=False):
        if method == "adaptive":
            raise DdifError("DPM_Solver.sample(method='adaptive'): the adaptive solver sizes every step from a norm of the iterate that would have to be read back "
                            "from the device each step; out of scope of the HIP path (use 'singlestep', 'singlestep_fixed' or 'multistep')")
        if method not in ("multistep", "singlestep", "singlestep_fixed"):
            raise ValueError("Got wrong method {}".format(method))
        if solver_type not in ("dpmsolver", "taylor"):
            raise ValueError("'solver_type' must be either 'dpmsolver' or 'taylor', got {}".format(solver_type))
        plain = method == "multistep" and solver_type == "dpmsolver" and self.algorithm_type == "dpmsolver++" and not denoise_to_zero and not return_intermediate
        if not plain or (self._guidance() is not None and self._fused_target() is not None):  # a guided run is a solver program whatever its method
            return self._sample_program(x, steps, t_start, t_end, order, skip_type, method, lower_order_final, denoise_to_zero, solver_type, return_intermediate)
        ns = self.noise_schedule
        t_0 = 1.0 / ns.total_N if t_end is None else t_end
        t_T = ns.T if t_start is None else t_start
        assert t_0 > 0 and t_T > 0 and steps >= order and 1 <= order <= 3
        ts = self.get_time_steps(skip_type, t_T, t_0, steps)
        assert ts.shape[0] - 1 == steps
        ords = []
        for k in range(steps):
            step = k + 1
            if step < order:
                ords.append(step)
            elif lower_order_final and steps < 10:
                ords.append(min(order, steps + 1 - step))
            else:
                ords.append(order)
        coefs = [self._update_coefs([ts[j].reshape(1) for j in range(max(0, k - 2), k + 1)], ts[k + 1].reshape(1), ords[k])
                 for k in range(steps)]
        fused = self._fused_target()
        if fused is not None and not return_intermediate and not denoise_to_zero:
            model, cond, clamp = fused
            B, _, H, W = x.shape
            plan = model.plan_for(B, H, W, x.device)
            plan.set_objective(self._model_fn.ddif["model_type"], plan.objective[1])  # the model_type branch of model_wrapper (reference :296-303) runs in dpm_x0_kernel
            if clamp == "dynamic":  # the two attributes are read here, at call time, as the reference's dynamic_thresholding_fn reads them
                plan.set_threshold("solver", float(self.dynamic_thresholding_ratio), float(self.thresholding_max_val))
                clamp = None
            else:
                plan.set_threshold("off")
            plan.set_tiling(None)  # the solver runs on independent tiles (a tiled DDPM / DDIM run may have left the cached plan tiled)
            plan.set_cond(cond)
            tabs = dict(n_evals=steps, order=order,
                        t_model=[float((ts[k] - 1.0 / ns.total_N) * 1000.0) for k in range(steps)],
                        alpha=[float(ns.marginal_alpha(ts[k].reshape(1))) for k in range(steps)],
                        sigma=[float(ns.marginal_std(ts[k].reshape(1))) for k in range(steps)],
                        ord=ords, cx=[c["cx"] for c in coefs], a_phi1=[c["a_phi1"] for c in coefs],
                        inv_r0=[c["inv_r0"] for c in coefs], inv_r1=[c["inv_r1"] for c in coefs],
                        r0_frac=[c["r0_frac"] for c in coefs], inv_r01=[c["inv_r01"] for c in coefs],
                        a_phi2=[c["a_phi2"] for c in coefs], a_phi3=[c["a_phi3"] for c in coefs])
            with torch.no_grad():
                return plan.sample_dpmpp(tabs, x, clamp)
        # generic loop: same algorithm, the model is called once per evaluation (reference :1179-1221)
        with torch.no_grad():
            models: List[torch.Tensor] = []
            for k in range(steps):
                models = (models + [self.model_fn(x, ts[k].reshape(1))])[-3:]
                x = self._apply_update(x, models, coefs[k], ords[k])
                if self.correcting_xt_fn is not None:
                    x = self.correcting_xt_fn(x, ts[k + 1].reshape(1), k + 1)
        return x

    def _sample_program(self, x, steps, t_start, t_end, order, skip_type, method, lower_order_final, denoise_to_zero, solver_type, return_intermediate):
        """Everything beyond the plain multistep DPM-Solver++ run: singlestep / singlestep_fixed, solver_type="taylor", algorithm_type="dpmsolver", the final
        denoise, intermediates.  One library call (ddif_plan_sample_dpm) on a solver program when the run can be fused, else the reference's loop (:1179-1249)
        over the update methods above."""
        ns = self.noise_schedule
        t_0 = 1.0 / ns.total_N if t_end is None else t_end
        t_T = ns.T if t_start is None else t_start
        assert t_0 > 0 and t_T > 0, "Time range needs to be greater than 0. For discrete-time DPMs, it needs to be in [1 / N, 1], where N is the length of betas array"
        fused = self._fused_target()
        if fused is not None:
            ops = self._build_program(steps, order, skip_type, method, lower_order_final, denoise_to_zero, solver_type, return_intermediate, t_T, t_0)
            model, cond, clamp = fused
            guidance = self._guidance()
            B, _, H, W = x.shape
            plan = model.plan_for(B if guidance is None else 2 * B, H, W, x.device)  # guided: the network's batch is [unconditional; conditional] (:334-337)
            plan.set_objective(self._model_fn.ddif["model_type"], plan.objective[1])
            if clamp == "dynamic":
                plan.set_threshold("solver", float(self.dynamic_thresholding_ratio), float(self.thresholding_max_val))
                clamp = None
            else:
                plan.set_threshold("off")
            plan.set_tiling(None)
            with torch.no_grad():
                if guidance is None:
                    plan.set_cond(cond)
                    out, inter = plan.sample_dpm(ops, self.algorithm_type, x, clamp)
                else:
                    plan.set_cond(torch.cat([guidance[1], cond]))
                    out, inter = plan.sample_dpm_guided(ops, self.algorithm_type, guidance[0], x, clamp)
            return (out, list(inter.unbind(0))) if return_intermediate else out
        intermediates = []
        with torch.no_grad():
            if method == "multistep":
                assert steps >= order
                timesteps = self.get_time_steps(skip_type, t_T, t_0, steps)
                assert timesteps.shape[0] - 1 == steps
                ords = self._multistep_orders(steps, order, lower_order_final)
                step = 0
                t = timesteps[step]
                t_prev_list = [t]
                model_prev_list = [self.model_fn(x, t)]
                if self.correcting_xt_fn is not None:
                    x = self.correcting_xt_fn(x, t, step)
                if return_intermediate:
                    intermediates.append(x)
                for step in range(1, steps + 1):
                    t = timesteps[step]
                    o = ords[step - 1]
                    x = self.multistep_dpm_solver_update(x, model_prev_list, t_prev_list, t, o, solver_type=solver_type)
                    if self.correcting_xt_fn is not None:
                        x = self.correcting_xt_fn(x, t, step)
                    if return_intermediate:
                        intermediates.append(x)
                    if step < steps:  # the final model value is never needed (:1219-1221)
                        t_prev_list = (t_prev_list + [t])[-3:]
                        model_prev_list = (model_prev_list + [self.model_fn(x, t)])[-3:]
            else:
                for step, (s, t, o, r1, r2) in enumerate(self._singlestep_schedule(steps, order, skip_type, method, t_T, t_0)):
                    x = self.singlestep_dpm_solver_update(x, s, t, o, solver_type=solver_type, r1=r1, r2=r2)
                    if self.correcting_xt_fn is not None:
                        x = self.correcting_xt_fn(x, t, step)
                    if return_intermediate:
                        intermediates.append(x)
            if denoise_to_zero:
                t = torch.ones((1,)) * t_0
                x = self.denoise_to_zero_fn(x, t)
                if self.correcting_xt_fn is not None:
                    x = self.correcting_xt_fn(x, t, step + 1)
                if return_intermediate:
                    intermediates.append(x)
        return (x, intermediates) if return_intermediate else x
