/* libddif -- C ABI of the MI355X-native DDIF denoising hot path.
 *
 * The reference (294coder/Dif-PAN) has no FFI: its boundary for this path is a set of Python call signatures.
 * Each entry point below names the reference interface it stands in for (paths relative to the reference root).
 * The Python package dif-pan_amd/ddif binds these with ctypes and re-exposes the reference's
 * own classes on top: UNetSR3 (models/sr3_dwt.py:30-219), GaussianDiffusion (diffusion/diffusion_ddpm_pan.py:143-778),
 * NoiseScheduleVP / model_wrapper / DPM_Solver (solver/dpm_solver.py).
 *
 * Conventions
 *   - every function returns 0 on success or a negative ddif_status; it never throws and never aborts;
 *     ddif_last_error() returns the message of the calling thread's last failure.
 *   - tensors crossing the boundary are fp32, contiguous, NCHW (the reference's layout), device pointers unless a
 *     parameter says "host".  The library converts to its internal NHWC layout.
 *   - all device work is enqueued on the caller's stream (a hipStream_t passed as void*; NULL = default stream) and
 *     is asynchronous; the library never calls hipDeviceSynchronize.  Pointers are borrowed until that work ends.
 *   - handles are not thread-safe; one host thread per handle, one process per GPU.
 */
#ifndef DDIF_H_
#define DDIF_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define DDIF_API __attribute__((visibility("default")))
#else
#define DDIF_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ddif_status {
    DDIF_OK = 0,
    DDIF_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    DDIF_ERR_HIP = -2,         /* a HIP runtime call failed */
    DDIF_ERR_MISSING = -3,     /* a required weight was never loaded */
    DDIF_ERR_STATE = -4,       /* call order violated (e.g. sample before set_cond) */
    DDIF_ERR_RANGE = -5        /* an activation left the range of the plan's arithmetic (ddif_plan_range_status): the result of that call is not valid */
} ddif_status;

typedef struct ddif_net* ddif_net_t;   /* weights (repacked for the kernels) of one UNetSR3 */
typedef struct ddif_plan* ddif_plan_t; /* per-(B,H,W) workspaces, cond caches, launch program */

/* Constructor arguments of UNetSR3 (models/sr3_dwt.py:31-51) that shape the network. */
typedef struct ddif_net_cfg {
    int32_t in_channel, out_channel, inner_channel, lms_channel, pan_channel, norm_groups;
    int32_t n_channel_mults;
    int32_t channel_mults[8];
    int32_t n_attn_res;
    int32_t attn_res[8];
    int32_t res_blocks, image_size, self_condition;
} ddif_net_cfg;

/* ---- network ------------------------------------------------------------------------------------------------ */

/* UNetSR3.__init__ (models/sr3_dwt.py:31-167).  Unsupported configurations (norm_groups != 1, fourier features,
 * pred_var, inner_channel != 32, head dim != 16) fail with DDIF_ERR_INVALID -- there is no fallback path. */
DDIF_API int ddif_net_create(ddif_net_t* out, const ddif_net_cfg* cfg, int device);
DDIF_API void ddif_net_destroy(ddif_net_t net);

/* nn.Module.load_state_dict, one tensor at a time (checkpoint layout: SURVEY.md appendix C; utils/misc.py:89-122).
 * `key` is the reference state-dict key, `data` a HOST pointer to fp32 in the reference layout (OIHW / (out,in)).
 * The pseudo key "noise_level_mlp.0.freqs" (inner_channel/2 floats) overrides the positional-encoding
 * frequencies exp(-ln(1e4) * j / count) (models/sr3_dwt.py:229-236) so they are bit-identical to torch's. */
DDIF_API int ddif_net_load(ddif_net_t net, const char* key, const float* data, const int64_t* shape, int ndim);
/* Repack everything loaded so far for the kernels and upload.  Must follow the last ddif_net_load. */
DDIF_API int ddif_net_commit(ddif_net_t net, void* stream);
/* Training: rewrite the packed weights IN PLACE from DEVICE parameter tensors (reference layouts, fp32; n (key, pointer) pairs covering
 * every learnable tensor of the state dict) -- one launch on `stream`, no host copy.  Plans of this net stay valid.  The eval-only
 * merged decoder-FFN weights are NOT refreshed: after a refresh only train-mode plans (ddif_plan_create_train) may run until the next
 * ddif_net_load + ddif_net_commit (inference plans are refused).  Replaces nothing in the reference: there `optimizer.step()` writes
 * the tensors the next forward reads (diffusion_engine.py:238); here the kernels read a packed copy. */
DDIF_API int ddif_net_refresh(ddif_net_t net, int n, const char* const* keys, const float* const* params_dev, void* stream);
DDIF_API int64_t ddif_net_num_params(ddif_net_t net);

/* ---- plan ----------------------------------------------------------------------------------------------------- */

/* Workspaces and launch program for batches of B tiles of H x W (H, W multiples of 8). */
DDIF_API int ddif_plan_create(ddif_plan_t* out, ddif_net_t net, int B, int H, int W);
DDIF_API void ddif_plan_destroy(ddif_plan_t plan);

/* Everything in UNetSR3.forward that depends only on `cond` (models/sr3_dwt.py:389-391,540-546,563,661-663):
 * bilinear resizes, CondInjection.body -> FiLM scale/shift, FastAttnCondInjection kv -> softmax -> context.
 * cond: (B, 2C+4P, H, W) = cat[lms, pan, up(wavelets)] (diffusion_engine.py:221-228). */
DDIF_API int ddif_plan_set_cond(ddif_plan_t plan, const float* cond, void* stream);

/* UNetSR3.forward(x, time, cond, self_cond) (models/sr3_dwt.py:169-219) with cond as given to set_cond.
 * time: B floats on the HOST (long timesteps are passed as their float value); self_cond may be NULL (-> x). */
DDIF_API int ddif_plan_forward(ddif_plan_t plan, const float* x, const float* time_host, const float* self_cond, float* out,
                      void* stream);

/* Per-step coefficient tables of one sampling run, HOST arrays of n_steps floats in EXECUTION order
 * (first executed step first).  The caller derives them from the schedule buffers exactly as the reference does. */
typedef struct ddif_ddpm_tables {
    int32_t n_steps;
    const float* t_model;   /* value fed to the network as `time` */
    const float* coef_x0;   /* posterior_mean_coef1[t]                       (diffusion_ddpm_pan.py:316-320) */
    const float* coef_xt;   /* posterior_mean_coef2[t] */
    const float* coef_z;    /* [t != 0] * exp(0.5 * posterior_log_variance_clipped[t])          (:441-442) */
} ddif_ddpm_tables;

/* GaussianDiffusion.p_sample_loop (diffusion/diffusion_ddpm_pan.py:445-507) for pred_mode="x_start":
 *   img = x_T; for each step: x0 = net(img, t, cond, self_cond=img); x0 = clamp(x0 + lms, lo, hi) - lms (if do_clamp);
 *   img = coef_x0*x0 + coef_xt*img + coef_z*z.
 * x_T: (B,C,H,W) or NULL; noise: (n_steps,B,C,H,W) standard normals in execution order or NULL.  NULL draws from the
 * on-device counter-based generator keyed by (seed, draw index, tile0 + tile index, element), so a batch split
 * over several GPUs reproduces the single-GPU result.  out: (B,C,H,W) = final img (the residual to lms). */
DDIF_API int ddif_plan_sample_ddpm(ddif_plan_t plan, const ddif_ddpm_tables* tabs, const float* x_T, const float* noise,
                          uint64_t seed, uint64_t tile0, float clamp_lo, float clamp_hi, int do_clamp, float* out,
                          void* stream);

typedef struct ddif_ddim_tables {
    int32_t n_steps;
    const float* t_model;      /* the RESPACED index j (diffusion_ddpm_pan.py:661) */
    const float* sqrt_recip;   /* sqrt_recip_alphas_cumprod[j]      (:284-287) */
    const float* sqrt_recipm1; /* sqrt_recipm1_alphas_cumprod[j] */
    const float* sqrt_ap;      /* sqrt(alphas_cumprod_prev[j])      (:615-618) */
    const float* dir_coef;     /* sqrt(1 - alphas_cumprod_prev[j] - sigma^2) */
    const float* sigma;        /* [j != 0] * eta-sigma              (:609-613,619-620) */
} ddif_ddim_tables;

/* GaussianDiffusion.ddim_sample_loop after respacing (diffusion/diffusion_ddpm_pan.py:624-666,594-621);
 * self_cond is never passed (-> x); no clamp unless do_clamp. */
DDIF_API int ddif_plan_sample_ddim(ddif_plan_t plan, const ddif_ddim_tables* tabs, const float* x_T, const float* noise,
                          uint64_t seed, uint64_t tile0, float clamp_lo, float clamp_hi, int do_clamp, float* out,
                          void* stream);

/* One model evaluation of DPM-Solver++ (solver/dpm_solver.py:279-300,441-450): net(x, t_model, cond) -> eps ->
 * x0 -> image-space clamp corrector; x, x0_out: (B,C,H,W) in the library's INTERNAL layout handles below. */
typedef struct ddif_dpm_tables {
    int32_t n_evals;           /* model evaluations = steps */
    int32_t order;             /* 1..3 */
    const float* t_model;      /* (t - 1/N) * 1000, float                              (dpm_solver.py:285-286) */
    const float* alpha;        /* marginal alpha at each evaluation time */
    const float* sigma;        /* marginal std   at each evaluation time */
    /* update k (k = 0 .. n_evals-1) advances x from evaluation time k to time k+1 with order ord[k]: */
    const int32_t* ord;
    const float* cx;           /* sigma_t / sigma_prev                                  (:836,897) */
    const float* a_phi1;       /* alpha_t * expm1(-h) */
    const float* inv_r0;       /* 1 / r0      (orders 2,3) */
    const float* inv_r1;       /* 1 / r1      (order 3) */
    const float* r0_frac;      /* r0 / (r0 + r1) */
    const float* inv_r01;      /* 1 / (r0 + r1) */
    const float* a_phi2;       /* alpha_t * phi_2 */
    const float* a_phi3;       /* alpha_t * phi_3 */
} ddif_dpm_tables;

/* DPM_Solver.sample(method="multistep", algorithm_type="dpmsolver++") (solver/dpm_solver.py:1179-1221). */
DDIF_API int ddif_plan_sample_dpmpp(ddif_plan_t plan, const ddif_dpm_tables* tabs, const float* x_T, float clamp_lo,
                           float clamp_hi, int do_clamp, float* out, void* stream);

/* DPM_Solver.sample as a host-built SOLVER PROGRAM (solver/dpm_solver.py:1055-1253): singlestep and singlestep_fixed runs (:602-802, 1222-1240), both
 * algorithm types, both solver types, the final denoise (:549-553, 1243-1245) and the intermediates (:1190-1191, 1239-1240, 1248-1249).  The program is a flat
 * list of ops over DDIF_DPM_NUM_REGS state registers (iterates; register 0 holds x_T at the start) and DDIF_DPM_NUM_REGS model registers (model values):
 *   DDIF_DPM_EVAL           model[dst] = model value of net(state[src], t_model, cond).  Under DDIF_DPM_ALGO_DPMSOLVERPP that is the data prediction of
 *                           ddif_plan_sample_dpmpp (model_type branch, x0 = (x - sigma * eps) / alpha, then the image-space clamp or dynamic thresholding);
 *                           under DDIF_DPM_ALGO_DPMSOLVER the noise prediction alone (:435-439; the reference corrects inside data_prediction_fn only).
 *   DDIF_DPM_UPDATE         state[dst] = form(state[src], model[m[0..2]], c[]); dst == src is fine.  Forms, each in the reference's operation order with a
 *                           leading minus folded into its scalar:
 *                             DDIF_DPM_FORM_MULTI  the multistep update of ddif_plan_sample_dpmpp, order 1..3: c = cx, a1, inv_r0, inv_r1, r0_frac, inv_r01, a2, a3
 *                                                  (noise prediction :846-853, 902-911: cx = exp(log_alpha_t - log_alpha_prev), a1 = sigma_t * phi_1, a2 = -sigma_t * phi_2,
 *                                                  a3 = sigma_t * phi_3); m[0] newest
 *                             DDIF_DPM_FORM_LIN1   c0 * x - c1 * m0
 *                             DDIF_DPM_FORM_LIN2   (c0 * x - c1 * m0) + c2 * (c3 * (m1 - m2))      m = {m0, m1, m2}; c3 = 1 wherever the reference has no second factor
 *                             DDIF_DPM_FORM_TAY3   D1_0 = c3 * (m1 - m0), D1_1 = c4 * (m2 - m0), D1 = (c6 * D1_0 - c5 * D1_1) / c7, D2 = 2 * (D1_1 - D1_0) / c7,
 *                                                  ((c0 * x - c1 * m0) + c2 * D1) - c8 * D2          c3 = 1 / r1, c4 = 1 / r2, c5 = r1, c6 = r2, c7 = r2 - r1
 *   DDIF_DPM_FINAL_DENOISE  state[dst] = the data prediction WITH the corrector at state[src], under either algorithm (:549-553)
 *   DDIF_DPM_EMIT           the next (B,C,H,W) slice of inter_out = state[src]
 * One launch per evaluation behind the network (model value, corrector, store, and the update that follows it in the program); dynamic thresholding keeps its
 * selection launch in front.  The program is validated before anything is enqueued: registers in range and written before they are read, orders 1..3, EMIT only
 * with inter_out, do_clamp not together with DDIF_THRESHOLD_SOLVER -- DDIF_ERR_INVALID otherwise.  The sticky objective and threshold of the plan apply as in
 * ddif_plan_sample_dpmpp.  out = state[0] after the last op. */
#define DDIF_DPM_NUM_REGS 3
#define DDIF_DPM_ALGO_DPMSOLVERPP 0
#define DDIF_DPM_ALGO_DPMSOLVER 1
#define DDIF_DPM_EVAL 0
#define DDIF_DPM_UPDATE 1
#define DDIF_DPM_FINAL_DENOISE 2
#define DDIF_DPM_EMIT 3
#define DDIF_DPM_FORM_MULTI 1
#define DDIF_DPM_FORM_LIN2 2
#define DDIF_DPM_FORM_TAY3 3
#define DDIF_DPM_FORM_LIN1 4
typedef struct ddif_dpm_op {
    int32_t kind;                  /* DDIF_DPM_EVAL .. DDIF_DPM_EMIT */
    int32_t form, order;           /* UPDATE: DDIF_DPM_FORM_*; order of FORM_MULTI */
    int32_t src, dst;              /* registers, see above */
    int32_t m[3];                  /* UPDATE: model registers (unused ones: any value in range) */
    float t_model, alpha, sigma;   /* EVAL / FINAL_DENOISE: (t - 1/N) * 1000 and the marginal alpha / std at t */
    float c[9];                    /* UPDATE */
} ddif_dpm_op;
typedef struct ddif_dpm_program {
    int32_t n_ops;
    int32_t algorithm;             /* DDIF_DPM_ALGO_* */
    const ddif_dpm_op* ops;        /* HOST array */
} ddif_dpm_program;
DDIF_API int ddif_plan_sample_dpm(ddif_plan_t plan, const ddif_dpm_program* prog, const float* x_T, float clamp_lo, float clamp_hi, int do_clamp, float* out,
                                  float* inter_out /* nullable: [number of EMIT ops][B][C][H][W] */, void* stream);

/* The same solver programs under CLASSIFIER-FREE GUIDANCE (model_wrapper, solver/dpm_solver.py:330-338): every evaluation runs the network once on the doubled
 * batch x_in = cat([x, x]), t_in = cat([t, t]), c_in = cat([unconditional_condition, condition]) (:334-337), converts the whole output to a noise prediction by
 * the model_type branch (:296-303), and hands on  eps = eps_u + guidance_scale * (eps_c - eps_u)  (:338, in that operation order, contraction off).  Everything
 * behind it -- data prediction, image-space clamp or dynamic thresholding, every update form, the final denoise, the intermediates -- sees eps as it sees an
 * unguided noise prediction.
 *   - The plan's batch is 2 * Bg and ddif_plan_set_cond has been given [unconditional (Bg); conditional (Bg)].  x_T, out and every inter_out slice hold Bg images.
 *   - x_T is laid into both halves of state register 0; every update writes its result to both halves (they hold the same bits throughout: the network reads a
 *     state register as its batch); model registers use one half.  EMIT and the final store write one half.
 *   - The corrector is the CONDITIONAL sample's: the clamp reads the lms channels of the conditional half of cond, and dynamic thresholding computes one s_b per
 *     guided sample from the guided eps.
 *   - Launches per evaluation are those of ddif_plan_sample_dpm at the same plan batch: the guidance arithmetic rides in the evaluation launch (and in the
 *     selection launch of dynamic thresholding).  No host synchronisation.
 * Fails before anything is enqueued: an odd plan batch, a guidance_scale that is not finite or a NULL prog / x_T / out -> DDIF_ERR_INVALID; cond not set ->
 * DDIF_ERR_STATE; and the program validation of ddif_plan_sample_dpm.  guidance_scale == 1 is legal here (eps_u + (eps_c - eps_u), not bit-equal to eps_c): the
 * reference's shortcut to a single conditional evaluation (:331-332) is the caller's, who then uses ddif_plan_sample_dpm on a plan of batch Bg. */
DDIF_API int ddif_plan_sample_dpm_guided(ddif_plan_t plan, const ddif_dpm_program* prog, float guidance_scale, const float* x_T, float clamp_lo, float clamp_hi,
                                         int do_clamp, float* out, float* inter_out /* nullable: [number of EMIT ops][Bg][C][H][W] */, void* stream);

/* GaussianDiffusion.p_losses forward half (diffusion/diffusion_ddpm_pan.py:692-732), eval mode, pred_mode x_start:
 * x_t = a[b]*x0 + s[b]*noise; pred = net(x_t, t, cond, self_cond); returns pred (recon_x0). a, s, time: B floats each, HOST or DEVICE
 * memory (copied on `stream`: a training loop that draws t on the device hands them over without a host round trip). */
DDIF_API int ddif_plan_q_sample_forward(ddif_plan_t plan, const float* x0, const float* noise, const float* sqrt_ac_host,
                               const float* sqrt_1mac_host, const float* time_host, const float* self_cond,
                               float* pred, void* stream);

/* ---- objective: what the network predicts and which loss trains it ------------------------------------------------------ */

/* GaussianDiffusion(pred_mode=..., loss_type=...) (diffusion/diffusion_ddpm_pan.py:105-107,152-162).  Sticky per plan; a new plan has the engine's
 * configuration (DDIF_PRED_X_START, DDIF_LOSS_L1), under which every entry point above behaves exactly as before.  With another pred_mode the samplers
 * and the p_losses entry points treat the network output as the noise / v prediction:
 *   noise:  x0 = sqrt_recip_alphas_cumprod[t] * x_t - sqrt_recipm1_alphas_cumprod[t] * out      (:298-302 predict_start_from_noise)
 *   pred_v: x0 = sqrt_alphas_cumprod[t] * x_t - sqrt_one_minus_alphas_cumprod[t] * out          (:310-314 predict_start_from_v)
 * in front of the clamp (:366-375); ddif_plan_sample_dpmpp takes the matching model_type branch of model_wrapper (solver/dpm_solver.py:296-303:
 * "noise" eps = out, "v" eps = alpha * out + sigma * x) and needs no further tables.  DDPM / DDIM then need the two coefficient tables of the
 * conversion (the _ex entry points below); the plain entry points fail with DDIF_ERR_INVALID.  ddif_plan_num_launches does not change. */
#define DDIF_PRED_X_START 0
#define DDIF_PRED_NOISE 1
#define DDIF_PRED_V 2
#define DDIF_LOSS_L1 0   /* nn.L1Loss  (:152-153) */
#define DDIF_LOSS_L2 1   /* nn.MSELoss (:154-155) */
#define DDIF_LOSS_L1SSIM 2 /* HybridL1SSIM(channel=channels), weighted_r = (1.0, 0.1) (:194-195; utils/loss_utils.py:73-83); any pred_mode, with or without p2_weight */
DDIF_API int ddif_plan_set_objective(ddif_plan_t plan, int pred_mode, int loss_type);
DDIF_API int ddif_plan_get_objective(ddif_plan_t plan, int* pred_mode, int* loss_type);

/* HybridL1SSIM on plain tensors (utils/loss_utils.py:73-83 over LossWarpper :98-115, SSIMLoss :118-147 and _ssim :30-59), the kernels of the training step's
 * DDIF_LOSS_L1SSIM tail (csrc/kernels_ssimloss.h):
 *   loss = 0.0 + mean|img1 - img2| * w_l1 + (1 - mean(ssim_map(img1, img2))) * w_ssim                                   (fp32 scalars, this order)
 *   ssim_map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),  C1 = 0.01^2, C2 = 0.03^2       (data_range is unused, as there)
 *   mu = W*img, s11 = W*(img1 img1) - mu1^2, s22 = W*(img2 img2) - mu2^2, s12 = W*(img1 img2) - mu1 mu2
 * W* = the depthwise 11 x 11 Gaussian window (sigma 1.5; gaussian / create_window :11-27: fp32 values divided by their fp32 sum) with ZERO padding 5; the means
 * run over all B*C*H*W values.  img1, img2, d_img2: device tensors [B][C][H][W] (nhwc == 0) or [B][H][W][C] (nhwc != 0); any B, C, H, W >= 1.
 * loss_out: one float, host or device.  d_img2 (nullable): upstream * d loss / d img2.  The loss is symmetric in its arguments: the gradient with respect to
 * img1 is this call with the two swapped.  Bitwise reproducible (no atomics).  Allocates its scratch per call and synchronises the stream before returning. */
DDIF_API int ddif_l1ssim_loss(const float* img1, const float* img2, int B, int C, int H, int W, int nhwc, float w_l1, float w_ssim, float upstream, float* loss_out,
                              float* d_img2, void* stream);

/* The per-step coefficients of x0 = coef_xt * x_t - coef_out * out (HOST arrays of n_steps floats in execution order, gathered from the schedule
 * buffers like the other tables): (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod) for noise, (sqrt_alphas_cumprod,
 * sqrt_one_minus_alphas_cumprod) for pred_v (:298-314).  NULL / ignored under DDIF_PRED_X_START. */
typedef struct ddif_pred_tables {
    int32_t n_steps;
    const float* coef_xt;
    const float* coef_out;
} ddif_pred_tables;
/* p_sample_loop (:445-507) / ddim_sample_loop (:624-666) with p_mean_variance's pred_mode branch (:366-375).  In the DDIM loop eps is still
 * recomputed from the unclamped x0 (:605-606). */
DDIF_API int ddif_plan_sample_ddpm_ex(ddif_plan_t plan, const ddif_ddpm_tables* tabs, const ddif_pred_tables* pred, const float* x_T, const float* noise,
                                      uint64_t seed, uint64_t tile0, float clamp_lo, float clamp_hi, int do_clamp, float* out, void* stream);
DDIF_API int ddif_plan_sample_ddim_ex(ddif_plan_t plan, const ddif_ddim_tables* tabs, const ddif_pred_tables* pred, const float* x_T, const float* noise,
                                      uint64_t seed, uint64_t tile0, float clamp_lo, float clamp_hi, int do_clamp, float* out, void* stream);

/* ---- dynamic thresholding (Imagen) ------------------------------------------------------------------------------------- */

/* GaussianDiffusion(clamp_type="dynamic") (diffusion/diffusion_ddpm_pan.py:327-344, 391-399) and DPM_Solver(correcting_x0_fn="dynamic_thresholding")
 * (solver/dpm_solver.py:424-433).  Per step and per sample b:  s_b = max(quantile(|v_b|, ratio), max_val)  over all C*H*W values of the sample, with
 * torch.quantile's linear interpolation between the two neighbouring order statistics (rank fp32(ratio) * fp32(n - 1), evaluated as ATen does for fp32
 * input).  The quantile is an exact selection on the device (csrc/kernels_quantile.h), one launch in front of the update; nothing goes through the host.
 * Sticky per plan, like the objective:
 *   DDIF_THRESHOLD_OFF (default): every entry point behaves exactly as before.
 *   DDIF_THRESHOLD_DDPM: ddif_plan_sample_ddpm[_ex] with do_clamp != 0 replaces the absolute clamp by
 *       v = x0 + lms;  x0 = clamp(v, 0, s_b) / s_b - lms        (the LOWER BOUND IS 0, as in the reference, :341-343; clamp_lo / clamp_hi are ignored)
 *     and runs the update as its own launch behind the quantile kernel (the final conv's sampler epilogue cannot see a whole sample).  do_clamp == 0
 *     disables it too (p_sample_loop's clip_noise gates both clamps, :447).  No effect on ddif_plan_sample_ddim (ddim_sample never clamps dynamically).
 *   DDIF_THRESHOLD_SOLVER: ddif_plan_sample_dpmpp applies  x0 = clamp(x0, -s_b, s_b) / s_b  to every data prediction; do_clamp must be 0 (the
 *     image-space clamp is the other corrector, DDIF_ERR_INVALID otherwise).  No effect on the DDPM / DDIM loops.
 * ratio in [0, 1], max_val finite and >= 0 (both ignored for DDIF_THRESHOLD_OFF); DDIF_ERR_INVALID otherwise. */
#define DDIF_THRESHOLD_OFF 0
#define DDIF_THRESHOLD_DDPM 1
#define DDIF_THRESHOLD_SOLVER 2
DDIF_API int ddif_plan_set_threshold(ddif_plan_t plan, int mode, float ratio, float max_val);
DDIF_API int ddif_plan_get_threshold(ddif_plan_t plan, int* mode, float* ratio, float* max_val);
/* The stateless op (dynamic_thresholding_fn of both classes): x, out (nullable) device [B][n], s_out device [B].
 *   s_out[b] = max(quantile(|x_b|, ratio), max_val);  out = clamp(x, symmetric ? -s_b : 0, s_b) / s_b.   1 <= n < 2^31; launches on the current device. */
DDIF_API int ddif_dynamic_threshold(const float* x, int B, int64_t n, float ratio, float max_val, int symmetric, float* out, float* s_out, void* stream);

/* ---- overlapping tiles with per-step fusion ------------------------------------------------------------ */

/* The reference never tiles (diffusion_engine.py:373-377 feeds whole scenes); tiling is this build's way to scale, and these are its definitions --
 * stated here and in ddif/sharding.py, and used by every kernel and test.
 *   Grid, per axis: scene extent L, tile t, 0 <= overlap < t, L >= t.  stride = t - overlap;  n = 1 if L == t, else ceil((L - t) / stride) + 1;
 *     origin p_k = min(k * stride, L - t): the last tile is shifted flush with the border, so any L >= t works and a pixel may lie in more than two
 *     tiles per axis.  Tiles are numbered row-major (k = ky * nx + kx), scenes outermost (batch entry b = scene * ny * nx + k).
 *   Weight of tile k at a scene pixel (y, x) it covers: w_k = wy * wx, wy = min(y - py_k + 1, py_k + t - y), wx alike: small integers, exact in fp32.
 *   Blend of the values v_k of the covering tiles, in ascending k, fp32, no contraction:
 *       den = sum w_k (exact);   r_k = w_k / den;   out = v_0 + sum_{k >= 1} r_k * (v_k - v_0)   added in that order, v_0 = the first covering tile.
 *     A pixel with one cover is copied untouched, and equal inputs give exactly v_0: fusing what is already fused changes no bit. */
#if defined(__HIP__) && !defined(DDIF_EMU)
#define DDIF_INLINE static inline __attribute__((host)) __attribute__((device))
#else
#define DDIF_INLINE static inline
#endif
DDIF_INLINE int ddif_tile_count(int L, int t, int overlap) { return L == t ? 1 : (L - t + (t - overlap) - 1) / (t - overlap) + 1; }
DDIF_INLINE int ddif_tile_origin(int k, int L, int t, int overlap) { return k * (t - overlap) < L - t ? k * (t - overlap) : L - t; }
DDIF_INLINE int ddif_tile_weight(int y, int p, int t) { return y - p + 1 < p + t - y ? y - p + 1 : p + t - y; }

/* The B batch entries of a plan are the tiles of n_scenes scenes of scene_h x scene_w on the grid above; the tile is the plan's own H x W. */
typedef struct ddif_tiling {
    int32_t n_scenes, scene_h, scene_w, overlap;
} ddif_tiling;
/* SURVEY.md 8f-2 (no reference line: a design decision of this build).  Sticky per plan, like ddif_plan_set_threshold; t == NULL turns it off (the
 * default), and with it off every entry point behaves -- and launches -- exactly as before.  DDIF_ERR_INVALID unless B == n_scenes * ny * nx,
 * 0 <= overlap < min(H, W) and scene_h >= H, scene_w >= W.  Under tiling:
 *   - ddif_plan_sample_ddpm[_ex] / ddif_plan_sample_ddim[_ex] (all three objectives) take the unfused tail -- the update kernel as a launch of its own,
 *     as under DDIF_THRESHOLD_DDPM -- and fuse x_{t-1} over the overlaps after EVERY step (one more launch, in place: every element of a scene that
 *     lies in more than one tile is blended as above and written back to all its covers), so all covers of a pixel stay on one trajectory;
 *   - the library's noise is keyed by SCENE pixel, for x_T (draw 0) and every step's z alike: Philox element
 *         ((tile0 + scene) * C + c) * (scene_h * scene_w) + y * scene_w + x          (tile0 then counts scenes)
 *     so every cover of a pixel draws the same normal and the stitched noise does not depend on the overlap.  Host-supplied x_T / noise stay per
 *     tile, as without tiling: making them agree in the overlaps is the caller's business (cut them from a scene-sized field with ddif_tiles_cut);
 *   - DDIF_THRESHOLD_DDPM in ddif_plan_sample_ddpm[_ex] is DDIF_ERR_INVALID (a per-tile s_b would differ between the covers of a pixel);
 *   - ddif_plan_sample_dpmpp / _dpm / _dpm_guided are DDIF_ERR_INVALID: per-step fusion inside solver programs is not implemented -- sample the tiles
 *     independently (tiling off) and blend once at the end with ddif_tiles_blend ("final" blending);
 *   - ddif_plan_num_launches reports the tiled step: the step program + update + fusion (absent at overlap 0) + counter. */
DDIF_API int ddif_plan_set_tiling(ddif_plan_t plan, const ddif_tiling* t);
/* SURVEY.md 8f-2.  Scenes (S, C, Hs, Ws) -> tiles (S * ny * nx, C, tile_h, tile_w) on the grid above; NCHW device pointers; launches on the current device. */
DDIF_API int ddif_tiles_cut(const float* scene, int S, int C, int Hs, int Ws, int tile_h, int tile_w, int overlap, float* tiles, void* stream);
/* SURVEY.md 8f-2.  The inverse: tiles -> scenes by the blend above (the stitch of "final" blending; on the tiles of a fused run it reduces to copies). */
DDIF_API int ddif_tiles_blend(const float* tiles, int S, int C, int Hs, int Ws, int tile_h, int tile_w, int overlap, float* scene, void* stream);

/* Per-sample rows of p_losses beyond sqrt_ac / sqrt_1mac (B floats each, HOST or DEVICE like those):
 *   recon_xt, recon_out: x0 = recon_xt[b] * x_t - recon_out[b] * prediction (:708-713, :724, :735), the schedule pair of ddif_pred_tables gathered at t;
 *     required unless the plan predicts x_start;
 *   p2_weight: p2_loss_weight[t_b] (:762-764).  loss_func has already reduced to a scalar there, so the weighting is loss * mean_b(p2_weight[t_b]):
 *     one factor on the loss and on its gradient.  NULL = no weighting (p2_loss_weight_gamma = 0). */
typedef struct ddif_objective_rows {
    const float* recon_xt;
    const float* recon_out;
    const float* p2_weight;
} ddif_objective_rows;
/* ddif_plan_q_sample_forward under the plan's objective: `pred` (nullable) = the raw network output, `recon` (nullable) = the x0 rebuilt from it -- what
 * the self-conditioning pass feeds back (:702-714). */
DDIF_API int ddif_plan_q_sample_forward_ex(ddif_plan_t plan, const float* x0, const float* noise, const float* sqrt_ac_host, const float* sqrt_1mac_host,
                                           const float* time_host, const float* self_cond, const ddif_objective_rows* rows, float* pred, float* recon,
                                           void* stream);

/* ---- either side of the denoising loop ---------------------------------------------------------------------------- */

/* Cond assembly of the engine, fused with the level-1 Haar analysis the reference does with PyWavelets on the CPU at
 * dataset construction (dataset/pan_dataset.py:73-81,127-142; dataset/hisr.py:48-59; diffusion_engine.py:221-228,441-444):
 *   cond = cat[lms, pan, bilinear_up2([LL(lms), details(pan)])] / division        -> (B, 2C+4P, H, W)
 * lms_raw (B,C,H,W), pan_raw (B,P,H,W): device, raw sensor units; H, W even.
 * wavelet_order 0 = [LL, H, D, V] (PanCollection sets), 1 = [LL, H, V, D] (CAVE / Harvard). */
DDIF_API int ddif_cond_assemble(const float* lms_raw, const float* pan_raw, float division, int B, int C, int P, int H, int W,
                                int wavelet_order, float* cond_out, void* stream);

/* Validation metrics per image (utils/_metric_legacy.py:299-379 analysis_accu(choices=5) as called by
 * utils/metric.py:24-98 AnalysisPanAcc): out[b] = {SAM, ERGAS, PSNR (reference sign), CC}; gt, pred (B,C,H,W) device;
 * out: device, B*4 floats.  The reference's quirks are kept: last row / column dropped, pi = 3.14159256, SAM rounded to
 * 6 digits, PSNR = -20 log10(1/rmse). */
DDIF_API int ddif_metrics(const float* gt, const float* pred, int B, int C, int H, int W, float ergas_ratio, float* out, void* stream);
/* SSIM per image (out: B floats) as `skimage.metrics.structural_similarity(gt, pred, channel_axis=0)` computes it with library defaults
 * (reference utils/metric.py:153-166): 7x7 uniform window, K1 0.01, K2 0.03, sample covariance, mean over the image cropped by 3 pixels
 * per side and over the channels.  data_range: the reference passes none, for which skimage takes the float dtype range (-1, 1) -> 2.0.
 * PARITY UNPINNED: skimage is absent from the build image; the oracle restates the published algorithm. */
DDIF_API int ddif_ssim(const float* gt, const float* pred, int B, int C, int H, int W, float data_range, float* out, void* stream);

/* Q2n quality index per image -- Q4 on four bands, Q8 on eight: the index the paper's tables report next to SAM and ERGAS (Garzelli & Nencini 2009,
 * as in the pansharpening toolbox that the reference's `q2n` / `onions_quality`, utils/_metric_legacy.py:15-259, were ported from; its call site there is
 * commented out, :305).  gt, pred: (B, C, H, W) fp32 on the device, 1 <= C <= 8.  All block arithmetic is fp64.
 *   quantisation  v = rint(min(max(x * scale, 0), 65535)): the multiply in fp32, rounding half to even.  scale = 1 for raw sensor units, the dataset's
 *                 division for images normalised by it.  ROUNDING RULE: the MATLAB original's uint16() rounds, the Python port's
 *                 np.array(..., dtype=np.uint16) truncates; the two agree on integer-valued inputs, and this entry point rounds.
 *   bands         zero bands are appended up to Cp, the next power of two >= C (what :75-79 intends).
 *   blocks        ny = ceil(H / shift), nx = ceil(W / shift); block (j, i) reads rows j*shift .. j*shift + block - 1 and the matching columns, indices
 *                 beyond H - 1 / W - 1 clamped (edge replication: what the reference's padding :41-44 does wherever it runs; defined here for every size).
 *   per block     n = block^2, g_k / f_k the gt / pred bands:
 *                 s_k = mean(g_k);  t_k = population std of g_k, 1e-8 where that is 0 (norm_blocco, :99-104)
 *                 a_k = (g_k - s_k) / t_k + 1;   y_k = (f_k - s_k) / t_k + 1, or f_k - s_k + 1 (no division) where s_k == 0 exactly (:146-150)
 *                 z1 = (a_0, .., a_{Cp-1}), z2 = (y_0, -y_1, .., -y_{Cp-1}), m1 / m2 their per-band means over the block
 *                 T3 = n/(n-1) (mean|z1|^2 + mean|z2|^2 - |m1|^2 - |m2|^2);   bias = 2 |m1| |m2| / (|m1|^2 + |m2|^2)
 *                 T3 == 0: q = (0, .., 0, bias);  else q = n/(n-1) (mean(z1 (x) z2) - m1 (x) m2) bias 2 / T3, (x) = the recursion of onion_mult (:228-259)
 *   results       Q(block) = |q|_2 -> map_out (B, ny, nx) fp64, device, may be NULL;  Q2n(image) = the mean of its blocks -> q_out (B) fp64, device.
 * The kernel accumulates the integer moments the definition reduces to (exact in 64 bits), so results are bit-identical from run to run and an image's
 * map does not depend on the batch around it.
 * PARITY is pinned on the reference's own building blocks (norm_blocco, onion_mult, onion_mult2D, composed as above by tools/make_golden.py), NOT on the
 * return value of its `q2n`: :193 there takes `qu[:, :, i]` on an (N, bs, bs, C) array -- column i instead of band i -- so that two identical images
 * score 0.87 .. 2.06 per block instead of 1; it also raises for N > 1, for a band count that is no power of two and for sizes with 2 est > N + 1.
 * DDIF_ERR_INVALID: gt / pred / q_out NULL, C outside 1..8, block outside 2..64, shift outside 1..block, B / H / W < 1, scale not finite or <= 0. */
DDIF_API int ddif_q2n(const float* gt, const float* pred, int B, int C, int H, int W, float scale, int block, int shift, double* map_out, double* q_out,
                      void* stream);

/* Fused optimizer step of the training loop (diffusion_engine.py:237-241): global-norm gradient clipping
 * (utils/misc.py:25-36 -> clip_grad_norm_), torch.optim.AdamW.step and EmaUpdater.update (utils/optim_utils.py:43-58) as
 * three launches over a chunk table, whatever the number of tensors.  The handle owns the moment buffers (zero-initialised);
 * params / grads / ema are borrowed device pointers that must stay valid for the handle's lifetime (ema or its entries may
 * be NULL). */
typedef struct ddif_optim* ddif_optim_t;
DDIF_API int ddif_optim_create(ddif_optim_t* out, int n_tensors, const int64_t* sizes, float* const* params, const float* const* grads,
                               float* const* ema, int device);
/* Same with CALLER-OWNED moment buffers (exp_avg / exp_avg_sq of torch.optim.AdamW, one device array per tensor, borrowed for the handle's
 * lifetime and not zeroed): the optimizer state then lives where a checkpoint can save and restore it (reference diffusion_engine.py:333-340
 * saves weights only; full-state resume is SURVEY 8f-4). */
DDIF_API int ddif_optim_create_ex(ddif_optim_t* out, int n_tensors, const int64_t* sizes, float* const* params, const float* const* grads,
                                  float* const* ema, float* const* exp_avg, float* const* exp_avg_sq, int device);
DDIF_API void ddif_optim_destroy(ddif_optim_t h);
/* step: 1-based AdamW step count; max_grad_norm <= 0 disables clipping; ema_mode 0 = leave ema alone, 1 = ema <- p
 * (iteration <= start_iter), 2 = ema <- ema*decay + p*(1-decay); grad_norm_host (nullable) receives the pre-clip global
 * norm and makes the call synchronous. */
DDIF_API int ddif_optim_step(ddif_optim_t h, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                             float max_grad_norm, int ema_mode, float ema_decay, float* grad_norm_host, void* stream);

/* ---- training: train-mode plans, the native training step (ddif_plan_train_step below), building blocks ---- */

/* Train-mode network (UNetSR3 under .train(): nn.Dropout(p) between SiLU and conv of every ResnetBlock Block,
 * models/sr3_dwt.py:295, and DropPath(0.2) on every decoder FFN, :534,576).  A train-mode plan runs the same entry points
 * (ddif_plan_set_cond / ddif_plan_forward / ddif_plan_q_sample_forward) with the masks below applied; it starts with identity
 * masks.  Masks hold 0 or 1/(1-p) (what nn.Dropout multiplies by) / per-sample DropPath scales in {0, 1/(1-p)}. */
DDIF_API int ddif_plan_create_train(ddif_plan_t* out, ddif_net_t net, int B, int H, int W);
/* ---- native training step (reference diffusion_engine.py:230-233: `diff_loss, recon = diffusion(res, cond=cond); diff_loss.backward()`).
 * A train-mode plan also holds the REVERSE launch program of the whole denoiser.  Per iteration:
 *   ddif_net_refresh (weights changed)  ->  ddif_plan_set_cond  ->  masks (ddif_plan_train_random_masks / _set_dropout / _set_droppath)
 *   ->  ddif_plan_train_step: x_t = a x0 + s noise, train-mode forward, L1 loss against x0, backward.
 * ddif_plan_train_bind names the gradient tensors once: n (state-dict key, device pointer) pairs covering every learnable tensor, reference
 * layouts (conv (Cout,Cin,k,k), Linear (out,in), vectors); the step WRITES them (no accumulation).  loss_dev: one device float (mean
 * absolute error, F.l1_loss); pred (nullable): the network output (B,C,H,W).  a / s / t: arrays of B floats (sqrt(alpha_bar_t),
 * sqrt(1 - alpha_bar_t), t) in HOST or DEVICE memory (device: no synchronisation per iteration); self_cond nullable (B,C,H,W).  Deterministic: fixed-order reductions, no atomics. */
DDIF_API int ddif_plan_train_bind(ddif_plan_t plan, int n, const char* const* keys, float* const* grads_dev);
DDIF_API int ddif_plan_train_num_grads(ddif_plan_t plan, int* n);
/* the same on a GIVEN network input and target (no q_sample): what the gradient parity tests drive with the reference's own tensors */
DDIF_API int ddif_plan_train_forward_backward(ddif_plan_t plan, const float* x, const float* time_host, const float* self_cond, const float* target,
                                              float* loss_dev, float* pred, void* stream);
DDIF_API int ddif_plan_train_step(ddif_plan_t plan, const float* x0, const float* noise, const float* sqrt_ac_host, const float* sqrt_1mac_host,
                                  const float* time_host, const float* self_cond, float* loss_dev, float* pred, void* stream);
/* ddif_plan_train_step under the plan's objective (ddif_plan_set_objective; :722-766): target x0 / noise / v = a*noise - s*x0 (:304-308) by pred_mode,
 * F.l1_loss or F.mse_loss (gradient 2 (pred - target) / n) by loss_type, p2 weighting from rows->p2_weight.  pred (nullable): the network output;
 * recon (nullable): recon_x0 as the reference returns it -- from the prediction for noise (:724), from the TRUE v for pred_v (:734-735: the reference
 * passes the target there, so its recon_x0 is x_start up to rounding), the prediction itself for x_start. */
DDIF_API int ddif_plan_train_step_ex(ddif_plan_t plan, const float* x0, const float* noise, const float* sqrt_ac_host, const float* sqrt_1mac_host,
                                     const float* time_host, const float* self_cond, const ddif_objective_rows* rows, float* loss_dev, float* pred,
                                     float* recon, void* stream);
DDIF_API int ddif_plan_train_info(ddif_plan_t plan, int* n_dropout_sites, int* n_droppath_sites);  /* sites in execution order */
DDIF_API int ddif_plan_train_site(ddif_plan_t plan, int site, int* C, int* H, int* W);             /* mask shape (B, C, H, W) */
/* explicit masks (parity with a reference run whose masks were captured): mask (B,C,H,W) device; scales HOST [n_droppath][B] */
DDIF_API int ddif_plan_train_set_dropout(ddif_plan_t plan, int site, const float* mask, void* stream);
DDIF_API int ddif_plan_train_set_droppath(ddif_plan_t plan, const float* scales_host, void* stream);
/* fresh masks from the counter-based generator, keyed by (seed, site, tile0 + sample, element): independent of the batch split */
DDIF_API int ddif_plan_train_random_masks(ddif_plan_t plan, uint64_t seed, uint64_t tile0, float p_dropout, float p_droppath, void* stream);
/* read the masks in force back (what nn.Dropout / DropPath would have drawn): mask (B,C,H,W) device; scales DEVICE [n_droppath][B] */
DDIF_API int ddif_plan_train_get_dropout(ddif_plan_t plan, int site, float* mask, void* stream);
DDIF_API int ddif_plan_train_get_droppath(ddif_plan_t plan, float* scales_dev, void* stream);

/* The per-op entry points of round 2's op-by-op training tape (stateless forward / backward ops, ddif_convfwd_*, ddif_convbwd_*, ddif_blockbwd_*) are TEST-ONLY since
 * round 6: they stay in libddif.so as an independent cross-check of the reverse program above and are declared in include/ddif_testops.h. */

/* ---- measurement -------------------------------------------------------------------------------------------- */

/* Bracket EVERY launch of one denoising step out of `every_n_steps` with HIP events on the launch stream.  A step is either
 * profiled completely or not at all: when fewer than one step's worth of the `max_events` event pairs are left, profiling
 * stops, and `steps_recorded` says how many whole steps the sums cover.  Collect after the stream has been synchronised. */
DDIF_API int ddif_prof_begin(ddif_plan_t plan, int every_n_steps, int max_events);
typedef struct ddif_prof_result {
    int64_t launches;        /* timed launches */
    double total_ms;         /* sum of their durations */
    double total_flop;       /* algorithmic flops of the timed launches (2*M*N*K, unpadded) */
    double total_bytes;      /* algorithmic activation bytes read + written by them */
    char kernel_name[128];
    int64_t steps_recorded;  /* whole denoising steps the sums (and ddif_prof_classes) cover */
    int64_t launches_per_step; /* launches of the step program (event pairs one profiled step consumes) */
    double total_mfma_flop;  /* the same flops weighted by what the kernel ISSUES on the matrix pipe, in units of the dense 16-bit MFMA rate:
                              * x3 on the f16x2 path (three half products per fp32 product), x6 on bf16x3, x16 on the exact fp32 MFMA (which
                              * runs at 1/16 of that rate): total_mfma_flop / time / 2516.8 TF = the fraction of the matrix pipe's peak in use */
} ddif_prof_result;
DDIF_API int ddif_prof_collect(ddif_plan_t plan, ddif_prof_result* out);
/* Per-class breakdown of the same profiled steps (EVERY launch of a profiled step is bracketed): six entries -- 3x3 convs and
 * 1x1 convs of the levels with more than 256 pixels per sample, everything at the low-resolution levels, bottleneck
 * attention, softmax statistics, other.  Valid after ddif_prof_collect. */
typedef struct ddif_prof_class {
    int64_t launches;
    double total_ms, total_flop, total_bytes;
    char name[64];
    double total_mfma_flop;  /* as in ddif_prof_result */
} ddif_prof_class;
DDIF_API int ddif_prof_classes(ddif_plan_t plan, ddif_prof_class* out6);
/* launches of the step program (one denoising step = this many event pairs when profiled) and of the set_cond program */
DDIF_API int ddif_plan_num_launches(ddif_plan_t plan, int* step_launches, int* cond_launches);

/* flops / bytes of one denoising step and of set_cond for this plan (algorithmic, SURVEY.md 8d accounting) */
DDIF_API int ddif_plan_cost(ddif_plan_t plan, double* step_flop, double* step_bytes, double* cond_flop, double* cond_bytes);

/* Device memory of a plan: everything it allocated, of which `arena_bytes` hold the activations of the denoising-step program
 * (placed by liveness: a buffer is reused as soon as the last launch that touches its tensor has been enqueued); `unaliased_bytes`
 * is what the same activations would take with one buffer per tensor. */
DDIF_API int ddif_plan_memory(ddif_plan_t plan, int64_t* total_bytes, int64_t* arena_bytes, int64_t* unaliased_bytes);

/* Arithmetic of the convolutions of INFERENCE plans created afterwards (process-wide; also DDIF_MATH=bf16 in the environment):
 *   DDIF_MATH_SPLIT (default): fp32-class results -- f16x2 / bf16x3 split products or the exact fp32 MFMA; the parity configuration.
 *   DDIF_MATH_BF16: the THROUGHPUT variant BASELINE configs[1] names ("bf16"; the reference would get it from torch.autocast around
 *     models/sr3_dwt.py's nn.Conv2d calls): conv operands rounded once to bf16, one v_mfma_f32_32x32x16_bf16 product, fp32 accumulation;
 *     tensors in memory, GroupNorm statistics, attention and the sampler update stay fp32.  Not a parity configuration: bench.py reports
 *     its drift against the split path next to its rate.  Training plans ignore it.
 * Returns DDIF_ERR_INVALID for another value. */
#define DDIF_MATH_SPLIT 0
#define DDIF_MATH_BF16 1
DDIF_API int ddif_set_math_mode(int mode);
DDIF_API int ddif_get_math_mode(void);

/* Range guard of the f16x2 split (the default arithmetic of inference plans).  An IEEE half carries 2^4 x the activation, so the path is exact
 * only for |x| < 4094.  Behind a GroupNorm that bound is proven on the host from gamma / beta; a conv WITHOUT a GroupNorm in front (the decoder's
 * feed-forward pair, up-sampling convs, CondInjection.x_conv: models/sr3_dwt.py:528-533, 266-273, 380-396) stages its RAW input, which a trained
 * checkpoint (utils/misc.py:89-122 loads any) may push past it -- the half becomes inf and the output NaN.  Those launches therefore watch what
 * they stage and set a sticky per-plan flag.
 *   ddif_plan_range_status: synchronises `stream`, writes 1 to *overflow if a launch of this plan staged a value outside the range since the
 *     last call (and clears the flag), else 0, and returns DDIF_OK; called once per sampler / forward call by the Python layer, which then
 *     rebuilds the plan under ddif_set_f16_raw(0) and repeats the call.  A caller that does not want to fall back treats 1 as DDIF_ERR_RANGE.
 *   ddif_set_f16_raw(0): plans created afterwards keep convs on raw inputs on bf16x3 (full fp32 exponent range, six products instead of three);
 *     1 (default; DDIF_F16_RAW=0 in the environment for 0) = f16x2 with the watch.  GroupNorm-prologue convs are unaffected. */
DDIF_API int ddif_plan_range_status(ddif_plan_t plan, void* stream, int* overflow);
DDIF_API int ddif_set_f16_raw(int on);
DDIF_API int ddif_get_f16_raw(void);

/* TEST HOOK: cap the persistent grid (workgroups per conv / fused attention launch) of plans created afterwards; 0 removes the cap.
 * Results do not depend on the cap (work items are walked in a fixed order per workgroup and every reduction has a
 * fixed order); tests use it to make small cases walk many work items per workgroup, across sample boundaries,
 * which is the regime the B=64 benchmark configuration runs in. */
DDIF_API int ddif_debug_set_grid_cap(int max_workgroups);

DDIF_API const char* ddif_last_error(void);
DDIF_API const char* ddif_version(void);
/* 1 when built for the test-only host emulator (never shipped), 0 for the gfx950 build */
DDIF_API int ddif_is_emulated(void);

#ifdef __cplusplus
}
#endif
#endif /* DDIF_H_ */
