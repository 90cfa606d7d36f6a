// Plan construction (launch program of UNetSR3.forward, reference models/sr3_dwt.py:169-219 with the cond-only
// branches hoisted into set_cond) and the sampling loops (reference diffusion/diffusion_ddpm_pan.py:445-507,
// 624-666; solver/dpm_solver.py:1179-1221).
#include "ddif_plan.h"
#include <algorithm>
#include <cmath>
#include "kernels_conv.h"
#include "kernels_misc.h"
#include "attn_args.h"
#include "quantile_args.h"
#include "kernels_lafuse.h"

namespace ddif {

// ------------------------------------------------------------------------------------------------ conv variants
// The instantiations live in three translation units of their own (conv_variants.h: ddif_conv_k1.cpp = 1x1 convs, ddif_conv_k3.cpp = 3x3 convs with the plain
// epilogue, ddif_conv_k3e.cpp = 3x3 convs with an epilogue variant; ddif_xf.cpp = EPI_XF; ddif_lr.cpp = the low-resolution kernel): they build in parallel, and
// the plan builder below no longer recompiles 150 kernels when its logic changes.
// vec (kernels_conv.h VEC): 0 = scalar staging (stem with C = 31, cond convs with 9 / 11 / 34 / 40 input channels; only the
// prologue-free 3x3 / 1x1 kernels), 1 = float4 staging with one source per channel chunk, 2 = float4 staging with a
// per-thread source select (stem: cat[x, x] of 8 + 8 or 4 + 4 channels inside one 16-channel chunk).
// epi: EPI_* bits (kernels_conv.h) -- FiLM (CondInjection.x_conv), scalar output path (Cout % 4 != 0), residual add.
// Only the combinations the network uses are instantiated.
ConvVariant get_conv_variant(int ks, int stride, int ups, int ck, int pro, int cfg, int vec, int epi, int math) {
    if (cfg == 20 || cfg == 21)
        return (stride == 1 && !ups && vec == 1) ? get_lr_variant(ks, cfg == 20 ? 2 : 4, pro, epi, (math == MATH_F16X2 && pro == PRO_COLSM) ? MATH_BF16X3 : math) : ConvVariant();
    if (ks == 1) return get_conv_variant_k1(stride, ups, ck, pro, cfg, vec, epi);
    if (ks == 3) return epi ? get_conv_variant_k3e(stride, ups, ck, pro, cfg, vec, epi) : get_conv_variant_k3(stride, ups, ck, pro, cfg, vec);
    return ConvVariant();
}

static int num_cus();
// DDIF_X3=0: the exact-fp32 MFMA instantiation everywhere (bitwise an fmaf chain); covered by tests/test_env_switches.py
static int x3_enabled() { static const int v = env_int("DDIF_X3", 1); return v; }
// DDIF_F16=0: the split-operand convs stay on bf16x3 (six products) instead of f16x2 (three); tests/test_env_switches.py
static int f16_enabled() { static const int v = env_int("DDIF_F16", 1); return v; }
int g_math_mode = [] { const char* e = getenv("DDIF_MATH"); return (e && std::strcmp(e, "bf16") == 0) ? 1 : 0; }();
int g_f16_raw = env_flag("DDIF_F16_RAW", true);
// DDIF_LR_ROWS=0: the low-resolution 3x3 convs keep the general (pixel-item) staging where the row staging applies
static int lr_rows_enabled() { static const int v = env_int("DDIF_LR_ROWS", 1); return v; }
// DDIF_LAFUSE=0: the decoder's linear-attention half as three launches (q conv, column statistics, attn_out conv)
static int lafuse_enabled() { static const int v = env_int("DDIF_LAFUSE", 1); return v; }
// DDIF_XCD (bit mask, default 15 = all): XCD-contiguous work partition (ddif_dev.h wg_work_range) of 1 = the general conv kernel, 2 = the low-resolution kernel,
// 4 = the fused linear-attention block, 8 = the per-sample kernels (bottleneck attention block, gn_dw3x3 of the low levels).  The dispatcher puts workgroup b on
// XCD b % 8; with the map every kernel of the step gives XCD k the same eighth of the samples (tiles 8 k .. 8 k + 7 at B = 64), so halos, the cout tiles of a pixel
// tile and a consumer's input (written by the same XCD one launch earlier) meet in that XCD's private L2: 3.90 -> 3.76 ms per denoising step, same box
// (profiles/r05/k_xcd_ab.txt).  Results do not depend on it -- the partition only decides WHICH workgroup computes an item (tests/test_env_switches.py).
static int xcd_mask() { static const int v = env_int("DDIF_XCD", 15); return v; }
// DDIF_LA8=0: the decoder's linear-attention half at the 8 x 8 level as three launches (rounds 3-5) instead of the fused kernel of round 6 (kernels_lafuse8.h)
static int la8_enabled() { static const int v = env_int("DDIF_LA8", 1); return v; }
// DDIF_XF=0: CondInjection.x_conv + FiLM as a launch of its own everywhere (the form of rounds 1-5); tests/test_env_switches.py
static int xf_enabled() { static const int v = env_int("DDIF_XF", 1); return v; }
// DDIF_NB2=0: the f16x2 3x3 convs with >= 64 couts as 32-cout work items everywhere (the launch program of round 6) instead of 64-cout items (conv_variants.h
// cfg 67 / 68, round 7) where a launch has at least one such item per CU (the default, -1); DDIF_NB2=1: 64-cout items wherever an instantiation exists, whatever
// the item count (like DDIF_TILE16).  Bit-identical results, partials included: tests/test_conv_nb2.py
static int nb2_mode() { static const int v = env_int("DDIF_NB2", -1); return v; }
// DDIF_LR=0: the 8x8 / 16x16 levels on the general conv kernel (kernels_conv.h) as well; covered by tests/test_env_switches.py
static int lr_enabled() { static const int v = env_int("DDIF_LR", 1); return v; }
// Can a 64-cout ResnetBlock.block2 at an H x W level carry the next block's 64 -> 64 x_conv + FiLM (add_conv: only as a 64-cout work item, tiling 68)?  The plan
// builder asks before it makes the request: where the answer is no, nothing about the plan changes -- not even the order of its cond-only program.
static bool fold64_possible(int B, int H, int W, bool train, int math_mode) {
    // Only under DDIF_NB2=1, never by the default rule: the fold's y is no bit-for-bit twin of the 1x1 launch, so a site must fold at every batch size or at none (a
    // tile of a batch stays bit-equal to the tile run alone, tests/test_gpu_batch64.py) -- the item-count rule cannot select it, and folding at every batch size
    // would change the 132-launch program of small batches, which tests pin.  Measured at B = 64: -12.8 us per site (profiles/r11).
    if (nb2_mode() <= 0 || !xf_enabled() || train || math_mode != 0 || !x3_enabled() || !f16_enabled()) return false;
    (void)B;
    return W >= 16 && !(lr_enabled() && H * W <= 256);
}
// 16 x 16-pixel tiles on eight waves where they fill the CUs; below that (8-16 tiles per GPU: what one rank of a strong-scaling run holds) the four-wave
// 8 x 16 tiling gives twice the workgroups and every wave a SIMD to itself.  Results do not depend on the choice bit for bit: same products per pixel, and
// the 16 x 16 tilings write their statistics partials per 8 x 16 half tile (ConvArgs::st_halves).  DDIF_TILE16=1 / 0 forces one form.
static bool tile16_fills(long items16) {
    static const int tile16_env = env_int("DDIF_TILE16", -1);
    return tile16_env >= 0 ? tile16_env != 0 : items16 >= num_cus();
}
// what pick_cfg() decides from: the conv's shape and which arithmetic / kernel families it may take
struct CfgQuery {
    int ks, ck, pro, vec, stride, ups, Hout, Wout, Cout, B, cin, c0;
    bool allow_lr = true;  // the low-resolution kernel may be chosen
    bool exact = false;    // exact-fp32 MFMA asked for (ConvSpec::exact)
    bool f16ok = false;    // f16x2 is admissible for this conv
    bool b1 = false;       // bf16x1 (the throughput variant)
};
// cfg 20 / 21: the low-resolution kernel (kernels_lr.h) with 8x8 / 8x16 pixel tiles -- samples of <= 256 pixels whose
// channel counts fit its 16-channel slabs
static int pick_cfg(const CfgQuery& q) {
    const int ks = q.ks, ck = q.ck, pro = q.pro, vec = q.vec, stride = q.stride, ups_ = q.ups, Hout = q.Hout, Wout = q.Wout, Cout = q.Cout, B = q.B;
    const bool f16ok = q.f16ok, b1 = q.b1;
    const bool wide = (Wout >= 16) && stride == 1;
    const bool x3 = x3_enabled() && !q.exact;
    if (q.allow_lr && x3 && lr_enabled() && vec == 1 && stride == 1 && !ups_ && Hout * Wout <= 256 && Cout % 4 == 0 && q.cin % 16 == 0 && q.c0 % 16 == 0 &&
        ck == (ks == 3 ? 16 : 32))
        // (smaller tiles -- 4 x 8 pixels at the 8 x 8 level, 8 x 8 at 16 x 16: twice the workgroups, each with half the matrix work -- measured
        //  SLOWER, 1.375 -> 1.42 / 1.49 / 1.54 ms for the class, profiles/r04/f_lr_tiles_ab.txt: the items are latency chains that also stream the
        //  weights once per item; more of them only adds weight traffic)
        return (Hout <= 8 && Wout <= 8) ? 20 : 21;
    if (ks == 1 && vec == 1) {
        const int base = wide ? (Cout > 64 ? 3 : (Cout > 32 ? 1 : 0)) : (Cout > 64 ? 4 : 2);
        // 32-cout tiles stay on the exact instruction: with 12 MFMAs per stage the split only adds staging work
        // (measured: softmax_H(q).ctx.attn_out 64+64->32 @64^2 72 vs 58 us)
        if (x3 && ck == 32 && b1) return base + 52;  // 0,1,3,2,4 -> 52,53,55,54,56
        if (x3 && ck == 32 && base != 0) return base + 12;  // 1,3,2,4 -> 13,15,14,16
        return base;
    }
    if (ks == 3 && vec == 1 && stride == 1 && x3) {
        const bool f16 = f16ok && (pro == PRO_NONE || pro == PRO_GN_SILU);
        const long items16 = (long)B * ((Hout + 15) / 16) * ((Wout + 15) / 16) * ((Cout + 31) / 32);
        if (wide && Hout >= 32 && Wout >= 32 && tile16_fills(items16)) return b1 ? 47 : (f16 ? 27 : 7);
        if (wide || Cout <= 32) return b1 ? 48 : (f16 ? 28 : 8);
        return b1 ? 49 : (f16 ? 29 : 9);
    }
    static const bool s2_f16 = env_flag("DDIF_S2_F16", true);  // DDIF_S2_F16=0: the Downsample convs and the stem stay on the exact-fp32 tilings
    if (ks == 3 && vec == 1 && stride == 2 && !ups_ && x3 && f16ok && !b1 && s2_f16 && pro == PRO_NONE && Wout >= 16) return Cout <= 32 ? 28 : 29;
    if (ks == 3 && vec == 2 && stride == 1 && !ups_ && x3 && f16ok && !b1 && s2_f16 && pro == PRO_NONE && wide && Cout <= 32) {  // the stem
        const long items16 = (long)B * ((Hout + 15) / 16) * ((Wout + 15) / 16);
        return (Hout >= 32 && Wout >= 32 && tile16_fills(items16)) ? 27 : 28;
    }
    if (ks == 3 && vec == 1 && wide && !ups_) {
        const long items32 = (long)B * ((Hout + 15) / 16) * ((Wout + 15) / 16) * ((Cout + 31) / 32);
        if (Hout >= 32 && Wout >= 32 && items32 >= 2L * num_cus()) return (Cout % 64 == 0 && items32 >= 4L * num_cus()) ? 6 : 5;
    }
    if (wide) return 0;
    if (Cout <= 32 && stride == 1) return 0;
    return 2;
}

static int num_cus() {  // of the CURRENT device (plan entry points make the net's device current), cached per device
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (cache[dev] == 0) {
        int v = 0;
        cache[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    return cache[dev];
}
// Test hook (ddif_debug_set_grid_cap, include/ddif.h): caps the persistent grid of every conv launch of plans built
// afterwards, so that small parity cases walk several work items per workgroup across sample boundaries -- the
// regime the B=64 benchmark runs in.  0 = no cap.
int g_debug_grid_cap = 0;
static int wg_per_cu(size_t smem, int cap = 2) {
    // (3 or 4 persistent workgroups per CU measured slower for the 1x1 class of kernels_conv.h: 1.56 vs 1.46 ms per step)
    int byl = (int)((160 * 1024) / (smem ? smem : 1));
    if (byl < 1) byl = 1;
    return cap < byl ? cap : byl;
}

static inline dim3 ew_grid(size_t n) {
    size_t g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return dim3((unsigned)g);
}

// depthwise 3x3 launch: the channel-quad kernel whenever both sources have 4 | channels (every feature tensor), the scalar one for the 11-channel cond images
static inline void launch_dw3x3(hipStream_t s, const DwArgs& a) {
    const dim3 grid(a.B * a.tiles_x * a.tiles_y);
    if (a.c0 % 4 == 0 && a.c1 % 4 == 0) hipLaunchKernelGGL(dw3x3_q4_kernel, grid, dim3(256), 10 * 18 * 32 * sizeof(float), s, a);
    else hipLaunchKernelGGL(dw3x3_kernel, grid, dim3(256), 10 * 18 * 32 * sizeof(float), s, a);
}

// ------------------------------------------------------------------------------------------------ allocation
Plan::~Plan() {
    drop_graphs();
#ifndef DDIF_EMU
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    if (wg_stream) {
        (void)hipStreamSynchronize(wg_stream);
        (void)hipStreamDestroy(wg_stream);
    }
    if (side_read) {
        auto& ev = net->reader_events;
        ev.erase(std::remove(ev.begin(), ev.end(), side_read), ev.end());
        (void)hipEventDestroy(side_read);
    }
    if (wg_fork) (void)hipEventDestroy(wg_fork);
    if (wg_join) (void)hipEventDestroy(wg_join);
    for (auto e : a_free)
        if (e) (void)hipEventDestroy(e);
#endif
    for (void* p : allocs) (void)hipFree(p);
    for (auto e : ev0) (void)hipEventDestroy(e);
    for (auto e : ev1) (void)hipEventDestroy(e);
}

template <typename T>
int Plan::dalloc(T** p, size_t n) {
    void* q = nullptr;
    const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
    if (dry) {  // fake, never dereferenced
        *p = reinterpret_cast<T*>((uintptr_t)0x100000000000ull + dry_next);
        dry_next += bytes;
        return 0;
    }
    DDIF_HIPCHK(hipMalloc(&q, bytes));
    allocs.push_back(q);
    bytes_allocated += bytes;
    *p = reinterpret_cast<T*>(q);
    return 0;
}

int Plan::alloc_tensor(Tensor* t, int C_, int H_, int W_, bool step_act) {
    t->C = C_;
    t->H = H_;
    t->W = W_;
    t->st = nullptr;
    t->np = 0;
    if (!step_act || train_mode) return dalloc(&t->p, (size_t)B * H_ * W_ * C_);  // train: every activation lives until the reverse pass
    // activation of the step program: lives in the arena between its first and its last launch
    const size_t bytes = ((size_t)B * H_ * W_ * C_ * sizeof(float) + 255) & ~(size_t)255;
    if (dry) {
        if (int e = dalloc(&t->p, (size_t)B * H_ * W_ * C_)) return e;
        fake2id[t->p] = (int)lives.size();
        lives.push_back(Live{bytes, (int)step.size(), (int)step.size(), 0});
        return 0;
    }
    if (arena_next >= (int)lives.size() || lives[arena_next].bytes != bytes) return fail(DDIF_ERR_STATE, "plan arena: the two build passes disagree");
    t->p = reinterpret_cast<float*>(arena + lives[arena_next++].off);
    return 0;
}

void Plan::use(const void* p) {
    if (!dry || !p) return;
    auto it = fake2id.find(p);
    if (it == fake2id.end()) return;
    Live& l = lives[it->second];
    const int idx = (int)step.size();  // index of the launch being created
    if (idx > l.last) l.last = idx;
    if (idx < l.first) l.first = idx;
}

// TEST-ONLY stage tap (ddif_plan.h): `t` is complete and live behind the launch pushed last -- its producer, or, for a tensor produced earlier (a skip
// connection, a cond-only cache), a launch in front of its last reader.  Inference plans only; the dry pass's records are dropped with its programs.
void Plan::tap(const std::string& name, const Tensor& t, bool cond_only) {
    if (train_mode || !t.p) return;
    taps.push_back(Tap{name, t, (int)(cond_only ? pre.size() : step.size()) - 1, cond_only});
}

// Two passes over the same builder: the dry pass only records shapes and liveness, the real pass allocates.
int Plan::build() {
    math_mode = g_math_mode;
    f16_raw = g_f16_raw;
    final_fused = false;
    n_range_convs = 0;
    if (!d_range) {
        void* q = nullptr;
        DDIF_HIPCHK(hipMalloc(&q, 64));
        DDIF_HIPCHK(hipMemset(q, 0, 64));
        allocs.push_back(q);
        bytes_allocated += 64;
        d_range = reinterpret_cast<int*>(q);
    }
    if (train_mode) {  // no activation arena: the reverse pass reads the forward's tensors
        dry = false;
        tmods.clear();
        if (int e = net->build_dgrad_packs()) return e;
        if (int e = build_impl()) return e;
        return build_backward();
    }
    dry = true;
    if (int e = build_impl()) return e;
    // the network output is read by the sampler update / layout conversion AFTER the last launch of the program
    {
        auto it = fake2id.find(net_out.p);
        if (it != fake2id.end()) lives[it->second].last = 1 << 30;
    }
    // first-fit interval colouring in order of first use
    std::vector<int> order(lives.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lives[x].first < lives[y].first; });
    std::vector<int> placed;
    arena_bytes = 0;
    unaliased_bytes = 0;
    // DDIF_ARENA_PAD=<bytes> (development aid): every tensor reserves that much more, which shifts the relative placement of the tensors of a launch -- the probe behind
    // the "one ffn.0 instance of four takes 68-72 us instead of 47" question of rounds 5-6 (profiles/r06/arena_pad_probe.txt)
    static const size_t arena_pad = [] { const char* e = getenv("DDIF_ARENA_PAD"); return e ? (size_t)atoll(e) & ~(size_t)255 : (size_t)0; }();
    for (int id : order) {
        Live& l = lives[id];
        unaliased_bytes += l.bytes;
        const size_t need = l.bytes + arena_pad;
        std::vector<std::pair<size_t, size_t>> busy;  // address ranges of tensors alive at the same time
        for (int o : placed)
            if (!(lives[o].last < l.first || l.last < lives[o].first)) busy.emplace_back(lives[o].off, lives[o].off + lives[o].bytes + arena_pad);
        std::sort(busy.begin(), busy.end());
        size_t off = 0;
        for (auto& r : busy) {
            if (off + need <= r.first) break;
            if (r.second > off) off = r.second;
        }
        l.off = off;
        if (off + l.bytes > arena_bytes) arena_bytes = off + l.bytes;
        placed.push_back(id);
    }
    // reset everything the dry pass produced, then build for real
    dry = false;
    dry_next = 0;
    fake2id.clear();
    pre.clear();
    step.clear();
    taps.clear();
    cenc.clear();
    cdec.clear();
    drop_sites.clear();
    path_sites.clear();
    mask_recs = nullptr;
    n_mask_recs = 0;
    n_conv3 = n_conv3_x3 = n_conv3_f16 = n_conv3_b1 = 0;
    n_range_convs = 0;
    final_fused = false;
    tb_rows = 0;
    tb = tvals = nullptr;
    arena_next = 0;
    if (arena_bytes) {
        void* q = nullptr;
        DDIF_HIPCHK(hipMalloc(&q, arena_bytes));
        allocs.push_back(q);
        bytes_allocated += arena_bytes;
        arena = reinterpret_cast<char*>(q);
    }
    if (int e = build_impl()) return e;
    if (arena_next != (int)lives.size()) return fail(DDIF_ERR_STATE, "plan arena: the two build passes disagree");
    return 0;
}

// a conv kernel whose LDS need (variant + the launch's staging extra) passes 64 KiB: the attribute is per kernel function, set to the variant's maximum
static int raise_dynamic_lds(ConvKernelFn fn, size_t var_smem) {
    if (var_smem + 8192 > 64 * 1024)
        DDIF_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(var_smem + 8192)));
    return 0;
}

int Plan::add_conv(std::vector<Op>& prog, const ConvSpec& s, Tensor* out) {
    const PackedConv& pc = *s.pc;
    const int Hin = s.in0.H, Win = s.in0.W;
    const int Hc = s.ups ? 2 * Hin : Hin, Wc = s.ups ? 2 * Win : Win;
    const int Hout = s.stride == 2 ? (Hc - 1) / 2 + 1 : Hc, Wout = s.stride == 2 ? (Wc - 1) / 2 + 1 : Wc;
    const int c0 = s.in0.C, c1 = s.in1.C;
    if (c0 + c1 != pc.cin) return fail(DDIF_ERR_INVALID, "%s: input channels %d+%d != weight cin %d", s.name, c0, c1, pc.cin);
    if (pc.ks == 1 && (s.stride != 1 || s.ups)) return fail(DDIF_ERR_INVALID, "%s: 1x1 conv with stride/upsample", s.name);
    const int vec = (c0 % 4 != 0 || c1 % 4 != 0) ? 0 : ((c1 == 0 || c0 % pc.ck == 0) ? 1 : 2);
    if ((size_t)B * Hin * Win * (c0 > c1 ? c0 : c1) * 4 >= ((size_t)1 << 32) || (size_t)B * Hout * Wout * pc.cout * 8 >= ((size_t)1 << 32))
        return fail(DDIF_ERR_INVALID, "%s: a tensor of this batch reaches 4 GiB (32-bit offsets); split the batch", s.name);
    // f16x2 (kernels_conv.h MATH = 3): inference plans only (the half packs are not refreshed on the device), shared weights inside the
    // scaled half range (pc.w_f16), and for a GroupNorm prologue an output bound sqrt(N) max|gamma| + max|beta| inside the activation range
    bool f16ok = f16_enabled() && !train_mode && pc.w_f16 && !s.w_override && !s.exact;
    const bool raw_in = !(s.pro == PRO_GN || s.pro == PRO_GN_SILU || s.pro == PRO_GN_DW);  // nothing bounds the staged values: f16x2 only under the plan's range watch
    if (raw_in && !f16_raw) f16ok = false;
    if (f16ok && (s.pro == PRO_GN || s.pro == PRO_GN_SILU)) {
        auto ig = net->vec_absmax.find(s.gamma), ib = net->vec_absmax.find(s.beta);
        const double n = (double)(c0 + c1) * Hin * Win;
        f16ok = ig != net->vec_absmax.end() && ib != net->vec_absmax.end() && std::sqrt(n) * ig->second + ib->second < DDIF_F16_AMAX;
    }
    // bf16x1 (MATH = 4): the throughput variant, only under ddif_set_math_mode(DDIF_MATH_BF16); inference plans, shared weights
    const bool b1ok = math_mode == 1 && !train_mode && pc.w_b1 && !s.w_override && !s.exact;
    const bool f16ok0 = f16ok;
    if (b1ok) f16ok = false;
    const int epi = (s.film ? EPI_FILM : 0) | (s.res ? EPI_RES : 0) | (pc.cout % 4 != 0 ? EPI_SOUT : 0) | (s.silu ? EPI_SILU : 0) | (s.cso_mx ? EPI_COLST : 0);
    // one way to ask: choose(...) picks cfg (and the operand format that goes with it) for this conv's shape, variant(cfg, epi) looks the instantiation up
    CfgQuery q{pc.ks, pc.ck, s.pro, vec, s.stride, s.ups, Hout, Wout, pc.cout, B, c0 + c1, c1 ? c0 : c0 + c1};
    q.exact = s.exact;
    int cfg = 0, math = MATH_BF16X3;
    auto choose = [&](bool allow_lr, bool f16, bool b1) {
        q.allow_lr = allow_lr;
        q.f16ok = f16;
        q.b1 = b1;
        math = b1 ? MATH_BF16X1 : (f16 ? MATH_F16X2 : MATH_BF16X3);
        cfg = pick_cfg(q);
    };
    auto variant = [&](int cfg_, int epi_) { return get_conv_variant(pc.ks, s.stride, s.ups, pc.ck, s.pro, cfg_, vec, epi_, math); };
    choose(true, f16ok, b1ok);
    if (s.cso_mx && ((cfg != 20 && cfg != 21) || Hout > (cfg == 20 ? 8 : 16)))
        return fail(DDIF_ERR_INVALID, "%s: column statistics epilogue needs the low-resolution kernel and H <= 16", s.name);
    static const bool wres_env = env_flag("DDIF_WRES", true);  // DDIF_WRES=0: tiling 27 everywhere (tests/test_env_switches.py)
    if (cfg == 27 && wres_env && c0 == 32 && c1 == 0 && pc.cout <= 32 && pc.ck == 16 && pc.n_chunks == 2 && !s.w_override && s.w_bstride == 0 && variant(37, epi).fn)
        cfg = 37;
    ConvVariant var = variant(cfg, epi);
    // round 7: 64-cout work items (NB = 2) on the f16x2 tilings 27 / 28 -- the halo tile of a pixel tile is staged, normalised and split once per 64 couts, and the
    // launch walks half the stages.  The statistics partials stay per 32-cout block (ConvVariant::nbs), so outputs and partials are the bits of the 32-cout items and
    // the rule may look at the item count: only where every CU still gets an item (small batches keep the finer items).
    // Tiling 67 (eight waves) where the combination has it, else 68 (conv_variants.h: two eight-wave forms would spill); 27 -> 68 changes the pixel tile as well,
    // which the half-tile partials of round 6 already make bit-neutral.
    // Measured at B = 64 (profiles/r11): the sites without a prologue (ffn.0, ffn.3(ffn.2)) gain 1.8 - 2.8 us per launch on 67; the ResnetBlock convs of the 32 x 32
    // level LOSE 3.4 - 5 us on 68 (one four-wave workgroup per CU against one eight-wave one) and keep their 32-cout items -- except block2 where it can then carry the
    // next block's x_conv + FiLM (the 64 -> 64 fold below exists on 64-cout items only): 68 + fold replaces two launches, -12 us per site.  The fold changes the bits
    // of y, so it may not hang on the item count: it is taken under DDIF_NB2=1 only (fold64_possible above).
    const bool fold64 = nb2_mode() > 0 && s.xf && !train_mode && xf_enabled() && &prog == &step && pc.ks == 3 && pc.cout == 64 && s.tb_off < 0 && !s.samp && s.xf->pc && s.xf->w && s.xf->film &&
                        s.xf->pc->bias && s.xf->pc->cin == 64 && s.xf->pc->cout == 64 && get_xf_variant(s.stride, s.pro, 68, vec, epi, 2).fn;
    if ((cfg == 27 || cfg == 28) && var.fn && nb2_mode() != 0 && pc.cout % 64 == 0) {
        for (int c2 = cfg + 40; c2 <= 68; ++c2) {
            const int th = c2 == 67 ? 16 : 8;
            const long items64 = (long)B * ((Hout + th - 1) / th) * ((Wout + 15) / 16) * (pc.cout / 64);
            const ConvVariant v2 = variant(c2, epi);
            // (... and never on a launch of fewer than 64 items, whatever the device: the gain is measured on launches of 256 - 1024 items, and a device of a
            //  few CUs -- the host-emulated one reports 4 -- keeps the launch programs that tests/golden/plan_signature_emu.json pins)
            const bool pays = s.pro == PRO_NONE && items64 >= num_cus() && items64 >= 64;
            if ((nb2_mode() > 0 || pays) && v2.fn && (s.tb_off < 0 || variant(c2, epi | EPI_TBS).fn)) {
                cfg = c2;
                var = v2;
                break;
            }
        }
    }
    // the fallback ladder: low-resolution kernel -> general kernel (a prologue / epilogue combination the low-resolution kernel does not carry), and
    // bf16x1 -> the default math of this conv (a combination the throughput variant does not instantiate)
    auto general_kernel_if_no_lr = [&](bool f16, bool b1) {
        if (var.fn || (cfg != 20 && cfg != 21)) return;
        choose(false, f16, b1);
        var = variant(cfg, epi);
    };
    general_kernel_if_no_lr(f16ok, b1ok);
    if (!var.fn && b1ok) {
        f16ok = f16ok0;
        choose(true, f16ok, false);
        var = variant(cfg, epi);
        general_kernel_if_no_lr(f16ok, false);
    }
    if (!var.fn) return fail(DDIF_ERR_INVALID, "%s: no kernel variant (ks=%d stride=%d ups=%d ck=%d pro=%d cfg=%d vec=%d epi=%d)", s.name, pc.ks, s.stride, s.ups, pc.ck, s.pro, cfg, vec, epi);
    // round 6: a low-resolution 3x3 conv whose tile spans the whole image width (the 8x8 / 16x16 levels of a 64x64 tile) stages by rows (kernels_lr.h ROWS): same
    // results, ~1.3 us less instruction issue per launch.  DDIF_LR_ROWS=0: the general staging everywhere (tests/test_env_switches.py)
    bool lr_rows = false;
    if (var.lr && !var.b1 && pc.ks == 3 && Win == var.tw && Wout == Win && Hout == Hin && lr_rows_enabled()) {
        const ConvVariant vr = get_lr_variant(3, cfg == 20 ? 2 : 4, s.pro, epi, var.f16 ? MATH_F16X2 : MATH_BF16X3, true);
        if (vr.fn && vr.smem == var.smem) {
            var = vr;
            lr_rows = true;
        }
    }
    // round 6: the next block's x_conv + FiLM as a second output of this conv (kernels_conv.h EPI_XF) -- where the chosen f16x2 tiling has such an instantiation
    // and one wave holds all 32 couts of its pixels; otherwise the request is left undone and the caller emits the 1x1 launch as before
    bool xf = false;
    // round 7: ... or both 32-cout blocks of its pixels, as a 64-cout item (cfg 68): the 64 -> 64 x_conv of the second level's blocks
    const bool xf32 = pc.cout == 32 && s.xf && s.xf->pc && s.xf->pc->cin == 32 && (s.xf->pc->cout == 32 || s.xf->pc->cout == 64);
    const bool xf64 = pc.cout == 64 && cfg == 68 && s.xf && s.xf->pc && s.xf->pc->cin == 64 && s.xf->pc->cout == 64;
    if (s.xf && !train_mode && xf_enabled() && var.f16 && !var.lr && pc.ks == 3 && (xf32 || xf64) && !s.ups && s.tb_off < 0 && !s.samp && s.xf->w && s.xf->film &&
        s.xf->pc->bias && &prog == &step) {
        const ConvVariant vx = get_xf_variant(s.stride, s.pro, cfg, vec, epi, s.xf->pc->cout / 32);
        if (vx.fn && vx.smem == var.smem + (xf64 ? XF64_LDS_BYTES : 0)) {
            var = vx;
            xf = true;
        }
    }
    if ((s.pro == PRO_GN || s.pro == PRO_GN_SILU || s.pro == PRO_GN_DW) && (!s.in0.st || (s.in1.p && !s.in1.st) || !s.gamma || !s.beta))
        return fail(DDIF_ERR_STATE, "%s: GroupNorm prologue without producer statistics", s.name);
    if (&prog == &step) {  // liveness of everything this launch touches (dry pass)
        use(s.in0.p);
        use(s.in1.p);
        use(s.res);
        use(s.film);
        use(s.cs_mx);
        use(s.cs_sm);
        use(s.out_xn);
        use(s.cso_mx);
        use(s.cso_sm);
    }
    if (int e = alloc_tensor(out, pc.cout, Hout, Wout, &prog == &step)) return e;
    if (xf) {
        if (int e = alloc_tensor(&s.xf->out, s.xf->pc->cout, Hout, Wout, true)) return e;
    }
    ConvArgs a{};
    a.in0 = s.in0.p;
    a.in1 = s.in1.p;
    a.c0 = c0;
    a.c1 = c1;
    a.B = B;
    a.Hin = Hin;
    a.Win = Win;
    a.Hout = Hout;
    a.Wout = Wout;
    a.Cout = pc.cout;
    a.w = s.w_override ? s.w_override : (var.b1 ? pc.w_b1 : (var.f16 ? pc.w_f16 : (var.x3 ? pc.w_x3 : pc.w)));
    if (var.x3 && !s.w_override && !a.w) return fail(DDIF_ERR_STATE, "%s: split-operand variant without split weights", s.name);
    a.w_bstride = s.w_bstride;
    a.cs_mx = s.cs_mx;
    a.cs_sm = s.cs_sm;
    a.dw_w = s.dw_w;
    a.out_xn = s.out_xn;
    a.cso_mx = s.cso_mx;
    a.cso_sm = s.cso_sm;
    if (s.pro == PRO_GN_DW && (!s.dw_w || c0 + c1 > 256)) return fail(DDIF_ERR_INVALID, "%s: depthwise staging needs weights and <= 256 channels", s.name);
    if (s.pro == PRO_COLSM && (!s.cs_mx || !s.cs_sm || c0 % pc.ck != 0)) return fail(DDIF_ERR_INVALID, "%s: column-softmax prologue needs statistics and c0 %% %d == 0", s.name, pc.ck);
    a.n_chunks = var.wr ? 1 : pc.n_chunks;  // (resident weights: the whole input is one 32-channel stage)
    a.bias = (s.use_bias && pc.bias) ? pc.bias : zeros;
    a.tbias = zeros;  // strides 0: a row of zeros for every sample and step
    a.st0 = s.in0.st;
    a.np0 = s.in0.np;
    a.st1 = s.in1.st;
    a.np1 = s.in1.np;
    a.gamma = s.gamma;
    a.beta = s.beta;
    a.res = s.res;
    a.film = s.film;
    a.out = out->p;
    a.tiles_x = (Wout + var.tw - 1) / var.tw;
    a.tiles_y = (Hout + var.th - 1) / var.th;
    const int gy = (pc.cout + var.nt - 1) / var.nt;
    // the eight-wave 16 x 16 tilings write their statistics partials per 8 x 16 half tile, exactly as the four-wave 8 x 16 tiling of the same conv would (kernels_conv.h
    // ConvArgs::st_halves): the tiling may then depend on the number of work items without changing a single bit of what the consumer reads
    const bool st_halves = !var.lr && var.th == 16 && var.tw == 16 && var.nthr == 512;
    a.st_halves = st_halves ? 1 : 0;
    a.tiles_y8 = (Hout + 7) / 8;
    const int np_out = st_halves ? a.tiles_x * a.tiles_y8 : a.tiles_x * a.tiles_y;
    if (s.stats) {
        out->np = np_out * gy * var.nbs;  // (64-cout items of cfg 67 / 68: one partial per 32-cout block, the array of cfg 27 / 28)
        if (int e = dalloc(&out->st, (size_t)B * out->np * 2)) return e;
        a.st_out = out->st;
    }
    a.n_ct = gy;
    if (xf) {
        if (gy != 1 || !s.stats) return fail(DDIF_ERR_STATE, "%s: x_conv fold needs one cout tile and output statistics", s.name);
        s.xf->out.np = np_out;
        if (int e = dalloc(&s.xf->out.st, (size_t)B * s.xf->out.np * 2)) return e;
        a.xf_w = s.xf->w;
        a.xf_b = s.xf->pc->bias;
        a.xf_film = s.xf->film;
        a.xf_out = s.xf->out.p;
        a.xf_st = s.xf->out.st;
        a.xf_cout = s.xf->pc->cout;
        s.xf->done = true;
    }
    a.xcd = (xcd_mask() & (var.lr ? 2 : 1)) ? 1 : 0;
    if (var.f16 && raw_in) {  // (the kernels only look at it in their raw-input f16x2 instantiations)
        a.range_flag = d_range;
        ++n_range_convs;
    }
    // persistent launch: a few workgroups per CU, each walking a contiguous range of (cout tile, pixel tile) items
    const long items_per_sample = (long)a.tiles_x * a.tiles_y * gy;
    const long nwork = (long)B * items_per_sample;
    const int gy0 = (pc.cout + var.nt - 1) / var.nt;
    const size_t smem = var.lr ? var.smem : var.smem + conv_smem_extra(s.pro, var.wr ? 1 : pc.n_chunks, var.wr ? 32 : pc.ck, gy0 * var.nt, xf ? s.xf->pc->cout : 0);
    long cap = (long)num_cus() * wg_per_cu(smem, var.wg_cap);
    if (g_debug_grid_cap > 0 && g_debug_grid_cap < cap) cap = g_debug_grid_cap;
    const dim3 grid((unsigned)(nwork < cap ? nwork : cap), 1u);
    const dim3 block((unsigned)var.nthr);
    if (int e = raise_dynamic_lds(var.fn, var.smem)) return e;
    if (smem > var.smem + 8192) return fail(DDIF_ERR_INVALID, "%s: %d input channels exceed the GroupNorm staging area", s.name, c0 + c1);
    // convs with a time bias: in the samplers every sample shares the step's row (bias + row live in LDS); forward() /
    // q_sample_forward with one t per sample use the EPI_TBS instantiation (rows loaded per work item)
    ConvKernelFn fn_tbs = nullptr;
    if (s.tb_off >= 0) {
        const ConvVariant vt = variant(cfg, epi | EPI_TBS);
        if (!vt.fn || vt.smem != var.smem) return fail(DDIF_ERR_INVALID, "%s: no per-sample time-bias kernel variant", s.name);
        fn_tbs = lr_rows ? var.fn : vt.fn;  // (the low-resolution kernel reads its time-bias rows from memory either way: ddif_lr.cpp)
        if (int e = raise_dynamic_lds(fn_tbs, var.smem)) return e;
    }
    // the final conv: the same tiling with the DDPM / DDIM update in its epilogue (split-operand tilings, vector output path)
    ConvKernelFn fn_samp = nullptr;
    if (s.samp && !train_mode && epi == 0 && s.tb_off < 0 && &prog == &step) {
        const ConvVariant vs = variant(cfg, EPI_SAMP);
        if (vs.fn && vs.smem == var.smem) {
            fn_samp = vs.fn;
            if (int e = raise_dynamic_lds(fn_samp, var.smem)) return e;
            final_fused = true;
        }
    }
    // ... and with the noise / v prediction turned into x0 in front of the update (EPI_PRED: its own instantiation, ddif_plan_set_objective)
    ConvKernelFn fn_samp_pred = nullptr;
    if (fn_samp) {
        const ConvVariant vp = variant(cfg, EPI_SAMP | EPI_PRED);
        if (vp.fn && vp.smem == var.smem) {
            fn_samp_pred = vp.fn;
            if (int e = raise_dynamic_lds(fn_samp_pred, var.smem)) return e;
            final_fused_pred = true;
        }
    }
    const float* lms_p = lms.p;
    const bool dyn = s.dyn_input;
    const bool self_c = net->cfg.self_condition != 0;
    const int tb_off = s.tb_off;
    static const bool dump = getenv("DDIF_DUMP_PLAN") != nullptr;
    if (dump)
        fprintf(stderr, "[ddif plan] %-34s %-24s ks=%d s=%d u=%d  %3d+%3d -> %3d  @%3dx%-3d pro=%d epi=%d cfg=%d items=%ld grid=%u smem=%zu  in@%p out@%p\n", s.name, var.name, pc.ks, s.stride,
                s.ups, c0, c1, pc.cout, Hout, Wout, s.pro, epi, cfg, nwork, grid.x, smem, (const void*)s.in0.p, (const void*)out->p);
    Op op;
    op.name = var.name;
    {
        char lb[160];
        snprintf(lb, sizeof lb, "%s %dx%d %d+%d->%d @%dx%d cfg%d", s.name, pc.ks, pc.ks, c0, c1, pc.cout, Hout, Wout, cfg);
        op.label = lb;
    }
    op.flop = 2.0 * B * Hout * Wout * (double)pc.cout * (c0 + c1) * pc.ks * pc.ks;
    op.bytes = 4.0 * B * ((double)Hin * Win * (c0 + c1) + (double)Hout * Wout * pc.cout);
    if (xf) {  // + the folded 1x1 conv and its FiLM operands / output
        op.label += " + x_conv+FiLM";
        op.flop += 2.0 * B * Hout * Wout * (double)s.xf->pc->cin * s.xf->pc->cout;
        op.bytes += 4.0 * B * (double)Hout * Wout * 3.0 * s.xf->pc->cout;
    }
    op.cls = (Hout * Wout <= 256) ? 2 : (pc.ks == 3 ? 0 : 1);
    op.mfma_w = var.b1 ? 1 : (var.f16 ? 3 : (var.x3 ? 6 : 16));
    op.timed = op.cls == 0;
    if (pc.ks == 3 && &prog == &step) {
        ++n_conv3;
        if (var.x3) ++n_conv3_x3;
        if (var.f16) ++n_conv3_f16;
        if (var.b1) ++n_conv3_b1;
    }
    op.run = [a, var, fn_tbs, fn_samp, fn_samp_pred, lms_p, grid, block, smem, dyn, self_c, tb_off](hipStream_t st, const StepCtx& ctx) {
        ConvArgs aa = a;
        const dim3 g = grid;
        if (dyn) {
            if (self_c) {
                aa.in0 = ctx.sc;
                aa.in1 = ctx.x;
            } else {
                aa.in0 = ctx.x;
            }
        }
        if (tb_off >= 0) {
            aa.tbias = ctx.tb + tb_off;
            aa.tbias_stride = ctx.tb_stride;
            aa.step_ptr = ctx.step_ptr;
            aa.tb_rowstride = ctx.tb_rowstride;
        }
        if (fn_samp && ctx.samp_out) {  // DDPM / DDIM loop: x_{t-1} straight from the epilogue
            aa.s_img = ctx.x;
            aa.s_lms = lms_p;
            aa.s_out = ctx.samp_out;
            aa.s_run = reinterpret_cast<const SamplerRun*>(ctx.samp_run);
            aa.s_step_next = ctx.step_next;
            aa.s_kind = ctx.samp_kind;
            aa.step_ptr = ctx.step_ptr;
            hipLaunchKernelGGL(ctx.samp_pred ? fn_samp_pred : fn_samp, g, block, smem, st, aa);
            return;
        }
        hipLaunchKernelGGL((tb_off >= 0 && ctx.tb_stride != 0) ? fn_tbs : var.fn, g, block, smem, st, aa);
    };
    prog.push_back(std::move(op));
    return 0;
}

// ------------------------------------------------------------------------------------------------ program
namespace {
#define DDIF_TRY(x) do { if (int e__ = (x)) return e__; } while (0)

// One pass of the plan builder: the state UNetSR3.forward threads through its layers (reference models/sr3_dwt.py:169-219) and one method per stage.
// Plan::build_impl() below is the table of contents.  Every method appends launches to p.step (per denoising step) or p.pre (cond-only, run by set_cond); the
// ORDER of their alloc_tensor / dalloc / use() / push_back calls is part of the result (arena placement, tests/test_plan_signature.py).
struct PlanBuilder {
    Plan& p;
    const Net& net;
    const ddif_net_cfg& c;
    const bool train;
    const int B, Cl, Pn, nlev;
    std::vector<Op>&pre, &step;

    Tensor cur;                 // the chain tensor
    std::vector<Tensor> feats;  // skip connections
    std::vector<int> feat_mod;  // train: index in tmods of the module that produced each feature
    int lev = 0;
    // cond-only FiLM branch of an encoder block: body(cond) -> scale | shift (sr3_dwt.py:379-391); built when first asked for -- by the block itself, or one
    // layer earlier by the conv that folds the block's x_conv + FiLM into its epilogue (round 6)
    std::map<const Layer*, std::pair<Tensor, Tensor>> film_cache;  // block -> (hid, film)
    // the fold request a producer conv at index li (stem / Downsample / the last conv of a block) hands to add_conv: the NEXT layer must be an encoder block
    XfReq xf_req;          // of the layer being built (add_conv fills out / done)
    bool xf_have = false;  // the previous layer's producer has already written this block's y = FiLM(x_conv(.))
    Tensor xf_y;

    explicit PlanBuilder(Plan& plan)
        : p(plan), net(*plan.net), c(plan.net->cfg), train(plan.train_mode), B(plan.B), Cl(c.lms_channel), Pn(c.pan_channel), nlev(c.n_channel_mults), pre(plan.pre),
          step(plan.step) {}

    const float* V(const std::string& k) const {
        auto it = net.vec.find(k);
        return it == net.vec.end() ? nullptr : it->second;
    }
    const PackedConv* PC(const std::string& k) const {
        auto it = net.conv.find(k);
        return it == net.conv.end() ? nullptr : &it->second;
    }
    int need_conv(const std::string& k, const PackedConv** pc) const {
        *pc = PC(k);
        return *pc ? 0 : fail(DDIF_ERR_MISSING, "%s missing", k.c_str());
    }
    static int cls_small(int HW, int other) { return HW <= 256 ? 2 : other; }  // profiling class of an elementwise / per-sample launch
    // train: the record of one module of UNetSR3.forward for the reverse pass (ddif_train.cpp); the caller adds the module-specific tensors
    Plan::TrainMod& tmod(Plan::TrainMod::Kind kind, const std::string& key, Tensor in, Tensor out) {
        Plan::TrainMod m;
        m.kind = kind;
        m.key = key;
        m.in = in;
        m.out = out;
        p.tmods.push_back(m);
        return p.tmods.back();
    }

    // ---- boundary staging + sampler state
    int boundary_buffers() {
        const int H = p.H, W = p.W, C = p.C;
        DDIF_TRY(p.dalloc(&p.zeros, (size_t)1024));
        if (!p.dry) DDIF_HIPCHK(hipMemset(p.zeros, 0, 1024 * sizeof(float)));
        DDIF_TRY(p.alloc_tensor(&p.x_in, c.in_channel, H, W));
        DDIF_TRY(p.alloc_tensor(&p.sc_in, c.out_channel, H, W));
        DDIF_TRY(p.alloc_tensor(&p.lms, C, H, W));
        const size_t img_n = (size_t)B * H * W * C;
        for (int i = 0; i < 2; ++i) DDIF_TRY(p.dalloc(&p.img[i], img_n));
        for (int i = 0; i < 3; ++i) DDIF_TRY(p.dalloc(&p.mbuf[i], img_n));
        DDIF_TRY(p.dalloc(&p.io_nchw, (size_t)B * H * W * (c.in_channel > C ? c.in_channel : C)));
        DDIF_TRY(p.dalloc(&p.small, (size_t)4 * B + 64));
        return 0;
    }

    // ---- cond-only program (set_cond): lms and the resized cond images of every level
    int cond_program() {
        Plan* const plan = &p;
        const int H = p.H, W = p.W, CC = p.CC;
        p.cenc.resize(nlev);
        p.cdec.resize(nlev);
        {
            Op op;
            op.name = "lms_nhwc";
            Tensor lm = p.lms;
            const int BB = B, CCc = CC, HW = H * W, Cc = p.C;
            op.run = [plan, lm, BB, CCc, HW, Cc](hipStream_t s, const StepCtx&) {
                hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid((size_t)BB * HW * Cc), dim3(256), 0, s, (const float*)plan->cond_nchw, BB, CCc, HW, 0, Cc, lm.p);
            };
            pre.push_back(std::move(op));
        }
        for (int l = 0; l < nlev; ++l) {
            DDIF_TRY(p.alloc_tensor(&p.cenc[l], Cl + Pn, p.LH[l], p.LW[l]));
            DDIF_TRY(p.alloc_tensor(&p.cdec[l], Cl + 3 * Pn, p.LH[l], p.LW[l]));
            for (int which = 0; which < 2; ++which) {
                Tensor t = which ? p.cdec[l] : p.cenc[l];
                const int cbeg = which ? CC - (Cl + 3 * Pn) : 0;
                Op op;
                op.name = "cond_resize";
                const int BB = B, CCc = CC, HH = H, WW = W;
                op.bytes = 4.0 * B * t.C * ((double)H * W + (double)t.H * t.W);
                op.run = [plan, t, cbeg, BB, CCc, HH, WW](hipStream_t s, const StepCtx&) {
                    hipLaunchKernelGGL(resize_bilinear_kernel, ew_grid((size_t)BB * t.H * t.W * t.C), dim3(256), 0, s,
                                       (const float*)plan->cond_nchw, BB, CCc, HH, WW, cbeg, t.C, t.H, t.W, t.p);
                };
                pre.push_back(std::move(op));
            }
        }
        return 0;
    }

    // ---- ResnetBlock (sr3_dwt.py:300-330)
    // train mode: y = silu(GN(x)) * dropout mask is materialised (it is also what wgrad needs), conv2 runs on it
    int gn_silu_dropout(const std::string& rb, Tensor x, const float* g, const float* bt, Tensor* y) {
        if (!x.st || !g || !bt) return fail(DDIF_ERR_STATE, "%s: GroupNorm without producer statistics / affine", rb.c_str());
        p.use(x.p);
        DDIF_TRY(p.alloc_tensor(y, x.C, x.H, x.W, true));
        Plan::DropSite site{nullptr, x.C, x.H, x.W};
        DDIF_TRY(p.dalloc(&site.mask, (size_t)B * x.H * x.W * x.C));
        p.drop_sites.push_back(site);
        const int HW = x.H * x.W, Cc = x.C, BB = B;
        const int chunks = (HW * Cc / 4 + 256 * 8 - 1) / (256 * 8);
        Tensor yy = *y;
        Op op;
        op.name = "gn_silu_dropout";
        op.cls = cls_small(HW, 5);
        op.bytes = 12.0 * B * HW * Cc;
        op.run = [x, g, bt, site, yy, HW, Cc, BB, chunks](hipStream_t s, const StepCtx&) {
            hipLaunchKernelGGL(gn_silu_drop_kernel, dim3(chunks < 1 ? 1 : chunks, BB), dim3(256), 0, s, (const float*)x.p, (const double*)x.st, x.np, g, bt,
                               (const float*)site.mask, HW, Cc, yy.p);
        };
        step.push_back(std::move(op));
        return 0;
    }
    int resblock(const std::string& rb, Tensor in, Tensor* out, XfReq* xf = nullptr) {
        const PackedConv *c1 = PC(rb + ".block1.block.3"), *c2 = PC(rb + ".block2.block.3");
        if (!c1 || !c2) return fail(DDIF_ERR_MISSING, "%s: conv weights missing", rb.c_str());
        Tensor h1;
        ConvSpec s1;
        s1.pc = c1;
        s1.in0 = in;
        s1.pro = PRO_GN_SILU;
        s1.gamma = V(rb + ".block1.block.0.weight");
        s1.beta = V(rb + ".block1.block.0.bias");
        s1.tb_off = net.slot_off.at(rb);
        s1.stats = true;
        s1.name = "res.conv1";
        DDIF_TRY(p.add_conv(step, s1, &h1));
        ConvSpec s2;
        s2.pc = c2;
        s2.res = in.p;
        s2.stats = true;
        if (!train) {
            s2.in0 = h1;
            s2.pro = PRO_GN_SILU;
            s2.gamma = V(rb + ".block2.block.0.weight");
            s2.beta = V(rb + ".block2.block.0.bias");
            s2.xf = xf;
            s2.name = "res.conv2";
            return p.add_conv(step, s2, out);
        }
        // Dropout sits in block2 only (ResnetBlock.__init__, sr3_dwt.py:318-319): block1 keeps the fused GroupNorm + SiLU prologue
        Tensor y2;
        DDIF_TRY(gn_silu_dropout(rb, h1, V(rb + ".block2.block.0.weight"), V(rb + ".block2.block.0.bias"), &y2));
        s2.in0 = y2;
        s2.name = "res.conv2 (train)";
        DDIF_TRY(p.add_conv(step, s2, out));
        Plan::TrainMod& m = tmod(Plan::TrainMod::RES, rb, in, *out);
        m.t[0] = h1;
        m.t[1] = y2;
        m.mask = p.drop_sites.back().mask;
        m.slot = net.slot_off.at(rb);
        return 0;
    }

    // ---- SelfAttention (sr3_dwt.py:333-361)
    // 64-token tiles: GroupNorm -> qkv -> softmax(q k^T / sqrt(C)) v -> out + bias + x in ONE kernel, one workgroup per sample (kernels_attn.h)
    int attn_block(const std::string& ap, const PackedConv* cq, const PackedConv* co, Tensor in, Tensor* out) {
        p.use(in.p);
        DDIF_TRY(p.alloc_tensor(out, in.C, in.H, in.W, true));
        const int asplit = attn_block_split();  // workgroups (= statistics partials) per sample
        out->np = asplit;
        DDIF_TRY(p.dalloc(&out->st, (size_t)B * 2 * asplit));
        DDIF_TRY(attn_block_prepare());
        AttnBlockArgs a{};
        a.x = in.p;
        a.st = in.st;
        a.np = in.np;
        a.gamma = V(ap + ".norm.weight");
        a.beta = V(ap + ".norm.bias");
        a.wqkv = cq->w_x3;
        {   // qkv on f16x2 (three products) where the f16x2 conditions of a GroupNorm-prologue conv hold: half packs exist (|w| < 64), and the bound
            // sqrt(N) max|gamma| + max|beta| of GroupNorm's output stays inside the scaled half range; DDIF_ATTN_F16=0 keeps bf16x3 (tests/test_env_switches.py)
            static const bool af16 = env_flag("DDIF_ATTN_F16", true);
            auto ig = net.vec_absmax.find(a.gamma), ib = net.vec_absmax.find(a.beta);
            const bool okr = ig != net.vec_absmax.end() && ib != net.vec_absmax.end() &&
                             std::sqrt((double)in.C * in.H * in.W) * ig->second + ib->second < DDIF_F16_AMAX;
            // ... and the chosen DDIF_ATTN_NW / DDIF_ATTN_SPLIT form has an f16x2 instantiation (ddif_lr.cpp): the pointer says what the launch computes with
            a.wqkv_f16 = (af16 && f16_enabled() && cq->w_f16 && okr && attn_block_has_f16()) ? cq->w_f16 : nullptr;
        }
        a.wout = co->w_x3;
        a.bout = co->bias ? co->bias : p.zeros;
        a.scale = 1.0f / std::sqrt((float)in.C);  // 1/sqrt(C), not 1/sqrt(d)   (sr3_dwt.py:352)
        a.out = out->p;
        a.st_out = out->st;
        a.B = B;
        a.xcd = (xcd_mask() & 8) ? 1 : 0;
        if (!a.gamma || !a.beta) return fail(DDIF_ERR_MISSING, "%s: norm weights missing", ap.c_str());
        Op op;
        op.name = "attn_block";
        op.label = std::string("attn_block (GN + qkv ") + (a.wqkv_f16 ? "f16x2" : "bf16x3") + " + attention + out + residual) @8x8";
        if (getenv("DDIF_DUMP_PLAN"))  // (its own prefix: the `[ddif plan]` lines are the convs of add_conv, tools/plan_signature.py)
            fprintf(stderr, "[ddif attn] %-34s qkv=%s split=%d\n", ap.c_str(), a.wqkv_f16 ? "f16x2" : "bf16x3", asplit);
        op.cls = 3;
        op.flop = 2.0 * B * 64 * 128.0 * (384 + 128) + 4.0 * B * 8 * 64.0 * 64 * 16;
        op.bytes = 8.0 * B * 64 * 128;
        int ncu = num_cus();
        if (g_debug_grid_cap > 0 && g_debug_grid_cap < ncu) ncu = g_debug_grid_cap;  // test hook: workgroups walk several samples / query parts (grid-stride loop)
        op.run = [a, ncu, asplit](hipStream_t s, const StepCtx&) { attn_block_launch(a, a.B * asplit < ncu ? a.B * asplit : ncu, s); };
        step.push_back(std::move(op));
        p.tap(ap + ".out", *out);
        return 0;
    }
    int self_attention(const std::string& ap, Tensor in, Tensor* out) {
        const PackedConv *cq = PC(ap + ".qkv"), *co = PC(ap + ".out");
        if (!cq || !co) return fail(DDIF_ERR_MISSING, "%s: conv weights missing", ap.c_str());
        p.tap(ap + ".in", in);
        if (!train && in.H * in.W == 64 && in.C == 128 && x3_enabled() && lr_enabled() && cq->w_x3 && co->w_x3 && cq->ck == 32 && co->ck == 32 && in.st)
            return attn_block(ap, cq, co, in, out);
        // other sizes: three launches
        Tensor qkv, o;
        ConvSpec s1;
        s1.pc = cq;
        s1.in0 = in;
        s1.pro = PRO_GN;
        s1.gamma = V(ap + ".norm.weight");
        s1.beta = V(ap + ".norm.bias");
        s1.use_bias = false;
        s1.name = "attn.qkv";
        DDIF_TRY(p.add_conv(step, s1, &qkv));
        DDIF_TRY(p.alloc_tensor(&o, in.C, in.H, in.W, true));
        p.use(qkv.p);
        {
            Op op;
            op.name = "self_attn";
            op.cls = 3;
            const int n = in.H * in.W, Cc = in.C, BB = B;
            const float scale = 1.0f / std::sqrt((float)Cc);  // 1/sqrt(C), not 1/sqrt(d)   (sr3_dwt.py:352)
            op.flop = 4.0 * B * 8 * (double)n * n * 16;
            op.bytes = 4.0 * B * n * 4.0 * Cc;
            op.run = [qkv, o, n, Cc, BB, scale](hipStream_t s, const StepCtx&) {
                hipLaunchKernelGGL(self_attn_mfma_kernel, dim3((n + 63) / 64, 8, BB), dim3(64), 0, s, (const float*)qkv.p, n, Cc, scale, o.p);
            };
            step.push_back(std::move(op));
        }
        ConvSpec s2;
        s2.pc = co;
        s2.in0 = o;
        s2.res = in.p;
        s2.stats = true;
        s2.name = "attn.out";
        DDIF_TRY(p.add_conv(step, s2, out));
        p.tap(ap + ".out", *out);
        if (train) {
            Plan::TrainMod& m = tmod(Plan::TrainMod::ATTN, ap, in, *out);
            m.t[0] = qkv;
            m.t[1] = o;
        }
        return 0;
    }
    // ResnetBlocWithAttn's second half: attention on the chain tensor where the layer has one
    int attention_if(const Layer& L) {
        if (!L.attn) return 0;
        Tensor t2;
        DDIF_TRY(self_attention(L.p + ".attn", cur, &t2));
        cur = t2;
        return 0;
    }

    // ---- encoder
    int film_of(const Layer& Lb, int at_lev, Tensor* hid_out, Tensor* film_out) {
        auto it = film_cache.find(&Lb);
        if (it != film_cache.end()) {
            *hid_out = it->second.first;
            *film_out = it->second.second;
            return 0;
        }
        const std::string ci = Lb.p + ".cond_inj";
        Tensor hid, film;
        ConvSpec s;
        DDIF_TRY(need_conv(ci + ".body.0", &s.pc));
        s.in0 = p.cenc[at_lev];
        s.use_bias = false;
        s.stats = true;
        s.name = "film.body0";
        DDIF_TRY(p.add_conv(pre, s, &hid));
        ConvSpec s2;
        DDIF_TRY(need_conv(ci + ".body.3", &s2.pc));
        s2.in0 = hid;
        s2.pro = PRO_GN_SILU;
        s2.gamma = V(ci + ".body.1.weight");
        s2.beta = V(ci + ".body.1.bias");
        s2.name = "film.body3";
        DDIF_TRY(p.add_conv(pre, s2, &film));
        film_cache[&Lb] = std::make_pair(hid, film);
        *hid_out = hid;
        *film_out = film;
        return 0;
    }
    // fold-request bookkeeping around a producer conv: fold_begin() resets xf_req and, where the layer after downs[li] (at level next_lev) is an encoder block
    // with a register-GEMM pack, fills it in; the producer's ConvSpec::xf points at xf_req; fold_end() notes whether add_conv honoured it
    int fold_begin(size_t li, int next_lev, bool may_fold = true) {
        xf_req = XfReq();
        if (!may_fold || train || li + 1 >= net.downs.size()) return 0;
        const Layer& Ln = net.downs[li + 1];
        if (Ln.kind == L_STEM || Ln.kind == L_DOWN) return 0;
        const std::string ci = Ln.p + ".cond_inj";
        const PackedConv* px = PC(ci + ".x_conv");
        const float* wxf = V(ci + ".x_conv.xf");
        if (!px || !wxf) return 0;
        if (px->cin == 64 && !fold64_possible(B, cur.H >> (next_lev - lev), cur.W >> (next_lev - lev), train, p.math_mode)) return 0;
        Tensor hid, film;
        DDIF_TRY(film_of(Ln, next_lev, &hid, &film));
        xf_req.pc = px;
        xf_req.w = wxf;
        xf_req.film = film.p;
        return 0;
    }
    void fold_end() {
        xf_have = xf_req.done;
        xf_y = xf_req.out;
    }
    int stem(size_t li) {
        const Layer& L = net.downs[li];
        const PackedConv* pc = PC(L.p);
        if (!pc) return fail(DDIF_ERR_MISSING, "%s missing", L.p.c_str());
        ConvSpec s;
        s.pc = pc;
        s.dyn_input = true;
        if (c.self_condition) {
            s.in0 = p.sc_in;
            s.in1 = p.x_in;
        } else {
            s.in0 = p.x_in;
        }
        s.stats = true;
        s.name = "stem";
        DDIF_TRY(fold_begin(li, lev));
        s.xf = &xf_req;
        DDIF_TRY(p.add_conv(step, s, &cur));
        fold_end();
        if (train) tmod(Plan::TrainMod::STEM, L.p, Tensor(), cur);
        return 0;
    }
    int down(size_t li) {
        const Layer& L = net.downs[li];
        ConvSpec s;
        DDIF_TRY(need_conv(L.p + ".conv", &s.pc));
        s.in0 = cur;
        s.stride = 2;
        s.stats = true;
        s.name = "down";
        const Tensor din = cur;
        DDIF_TRY(fold_begin(li, lev + 1));
        s.xf = &xf_req;
        DDIF_TRY(p.add_conv(step, s, &cur));
        fold_end();
        ++lev;
        if (train) tmod(Plan::TrainMod::DOWN, L.p + ".conv", din, cur);
        return 0;
    }
    // train: xc = x_conv(x) is kept (FiLM's backward needs it), the modulation is a launch of its own
    int cond_injection_train(const std::string& ci, ConvSpec& s, Tensor hid, Tensor film, Tensor* y_out) {
        Tensor xc, y;
        s.name = "film.x_conv (train)";
        DDIF_TRY(p.add_conv(step, s, &xc));
        DDIF_TRY(p.alloc_tensor(&y, xc.C, xc.H, xc.W, true));
        const int HWl = xc.H * xc.W, Cc = xc.C, BB = B;
        const int chunks = tk::film_chunks(HWl, Cc);
        y.np = chunks;
        DDIF_TRY(p.dalloc(&y.st, (size_t)B * chunks * 2));
        Tensor yy = y;
        Op op;
        op.name = "film_apply";
        op.cls = cls_small(HWl, 5);
        op.bytes = 16.0 * B * HWl * Cc;
        op.run = [xc, film, yy, HWl, Cc, BB, chunks](hipStream_t st, const StepCtx&) { tk::film_apply(st, xc.p, film.p, BB, HWl, Cc, yy.p, yy.st, chunks); };
        step.push_back(std::move(op));
        // the cond image zero-padded to 4 | channels: input of body.0's weight gradient (cond-only, part of set_cond)
        if ((int)p.cenc_pad.size() < nlev) p.cenc_pad.resize(nlev);
        if (!p.cenc_pad[lev].p) {
            const int Cp = (p.cenc[lev].C + 3) & ~3;
            DDIF_TRY(p.alloc_tensor(&p.cenc_pad[lev], Cp, p.cenc[lev].H, p.cenc[lev].W));
        }
        Plan::TrainMod& m = tmod(Plan::TrainMod::FILM, ci, cur, y);
        m.t[0] = xc;
        m.t[1] = film;
        m.t[2] = hid;
        m.t[3] = p.cenc[lev];
        m.t[4] = p.cenc_pad[lev];
        m.lev = lev;
        *y_out = y;
        return 0;
    }
    // CondInjection (y = FiLM(x_conv(x)), sr3_dwt.py:379-391) + ResnetBlocWithAttn
    int encoder_block(size_t li) {
        const Layer& L = net.downs[li];
        const std::string ci = L.p + ".cond_inj";
        // cond-only: body(cond) -> FiLM scale|shift
        Tensor hid, film;
        DDIF_TRY(film_of(L, lev, &hid, &film));
        Tensor y;
        const bool y_folded = xf_have;  // the producer one layer up wrote y already (EPI_XF)
        xf_have = false;
        ConvSpec s;
        DDIF_TRY(need_conv(ci + ".x_conv", &s.pc));
        s.in0 = cur;
        if (train) {
            DDIF_TRY(cond_injection_train(ci, s, hid, film, &y));
        } else if (y_folded) {
            y = xf_y;
        } else {
            s.film = film.p;
            s.stats = true;
            s.name = "film.x_conv";
            DDIF_TRY(p.add_conv(step, s, &y));
        }
        // the block's last conv folds the NEXT block's x_conv + FiLM when nothing (attention) sits between them
        DDIF_TRY(fold_begin(li, lev, !L.attn));
        DDIF_TRY(resblock(L.p + ".res_block", y, &cur, (!train && !L.attn) ? &xf_req : nullptr));
        fold_end();
        return attention_if(L);
    }
    int mid_block(const Layer& L) {
        Tensor t1;
        DDIF_TRY(resblock(L.p + ".res_block", cur, &t1));
        cur = t1;
        return attention_if(L);
    }
    // train: the decoder-only half of the cond-only program ran on the side stream (set_cond): it must be complete from here on
    void join_side_stream() {
        Plan* const plan = &p;
        Op j;
        j.name = "join cond-only side work";
        j.run = [plan](hipStream_t s, const StepCtx&) {  // (not under a stream capture: the samplers join before they start capturing)
            if (plan->side_pending) {
                plan->train_join(s);
                plan->side_pending = false;
            }
        };
        step.push_back(std::move(j));
    }

    // ---- decoder
    int up(const Layer& L) {
        ConvSpec s;
        DDIF_TRY(need_conv(L.p + ".conv", &s.pc));
        s.in0 = cur;
        s.ups = 1;
        s.stats = true;
        s.name = "up";
        const Tensor uin = cur;
        DDIF_TRY(p.add_conv(step, s, &cur));
        --lev;
        if (train) tmod(Plan::TrainMod::UP, L.p + ".conv", uin, cur);
        return 0;
    }
    // what the stages of one FastAttnCondInjection block (sr3_dwt.py:495-577) share
    struct Dec {
        std::string ci;  // "<block>.cond_inj"
        Tensor skip;
        int skip_from = -1;  // train: index in tmods of the module that produced `skip`
        int fea = 0, d = 0, Hl = 0, Wl = 0, cd = 0;
        size_t pre_dec0 = 0;  // train: everything this block adds to the cond-only program from here on is decoder-only -> the side stream
        float* ctx = nullptr;  // inference: linear-attention context [B][8][d][d]
        Tensor kdw, kv;
        const float *pn_g = nullptr, *pn_b = nullptr, *q0w = nullptr;  // prenorm_x affine, q.0 depthwise weights
    };
    // ---- cond-only: kv -> softmax_W(k) -> context   (sr3_dwt.py:514-517,541,546,563)
    int decoder_context(Dec& D) {
        const int BB = B, fea = D.fea, d = D.d, Hl = D.Hl, Wl = D.Wl, cd = D.cd;
        D.pre_dec0 = pre.size();
        DDIF_TRY(p.alloc_tensor(&D.kdw, cd, Hl, Wl));
        {
            DwArgs a{};
            a.in0 = p.cdec[lev].p;
            a.c0 = cd;
            a.B = B;
            a.H = Hl;
            a.W = Wl;
            a.w = V(D.ci + ".kv.0.weight");
            if (!a.w) return fail(DDIF_ERR_MISSING, "%s.kv.0.weight missing", D.ci.c_str());
            a.out_dw = D.kdw.p;
            a.tiles_x = (Wl + 15) / 16;
            a.tiles_y = (Hl + 7) / 8;
            Op op;
            op.name = "kv.dw3x3";
            op.flop = 2.0 * 9 * B * Hl * Wl * cd;
            op.bytes = 8.0 * B * Hl * Wl * cd;
            op.run = [a](hipStream_t s, const StepCtx&) { launch_dw3x3(s, a); };
            pre.push_back(std::move(op));
        }
        ConvSpec s;
        DDIF_TRY(need_conv(D.ci + ".kv.1", &s.pc));
        s.in0 = D.kdw;
        s.name = "kv.1x1";
        DDIF_TRY(p.add_conv(pre, s, &D.kv));
        if (train) return 0;  // (the train-mode forward runs the attention core itself)
        float *kmx = nullptr, *ksm = nullptr, *ctx = nullptr;
        DDIF_TRY(p.dalloc(&kmx, (size_t)B * Hl * fea));
        DDIF_TRY(p.dalloc(&ksm, (size_t)B * Hl * fea));
        DDIF_TRY(p.dalloc(&ctx, (size_t)B * 8 * d * d));
        D.ctx = ctx;
        const Tensor kv = D.kv;
        {
            Op op;
            op.name = "k.softmax_stats";
            op.bytes = 8.0 * B * Hl * Wl * fea;
            op.run = [kv, kmx, ksm, fea, BB, Hl, Wl](hipStream_t s, const StepCtx&) {
                hipLaunchKernelGGL(softmax_stats_kernel, ew_grid((size_t)BB * Hl * fea), dim3(256), 0, s, (const float*)kv.p, 2 * fea, 0, fea, BB, Hl, Wl, 1, kmx, ksm);
            };
            pre.push_back(std::move(op));
        }
        {
            Op op;
            op.name = "linattn_ctx";
            op.flop = 2.0 * B * 8 * d * d * (double)Hl * Wl;
            op.bytes = 4.0 * B * Hl * Wl * 2.0 * fea;
            op.run = [kv, kmx, ksm, ctx, fea, d, BB, Hl, Wl](hipStream_t s, const StepCtx&) {
                hipLaunchKernelGGL(linattn_ctx_kernel, dim3(8, BB), dim3(256), 2 * 32 * d * sizeof(float), s, (const float*)kv.p, (const float*)kmx, (const float*)ksm, BB, Hl, Wl, fea, d, ctx);
            };
            pre.push_back(std::move(op));
        }
        return 0;
    }
    // xn = GN(cat[h, skip]), dwq = dw3x3(xn): the two-source arguments of dw3x3_kernel / gn_dw3x3_small_kernel (the caller adds its tiling / partition)
    DwArgs gn_dw_args(const Dec& D, Tensor dwq, Tensor xn) const {
        DwArgs a{};
        a.in0 = cur.p;
        a.c0 = cur.C;
        a.in1 = D.skip.p;
        a.c1 = D.skip.C;
        a.B = B;
        a.H = D.Hl;
        a.W = D.Wl;
        a.st0 = cur.st;
        a.np0 = cur.np;
        a.st1 = D.skip.st;
        a.np1 = D.skip.np;
        a.gamma = D.pn_g;
        a.beta = D.pn_b;
        a.w = D.q0w;
        a.out_dw = dwq.p;
        a.out_xn = xn.p;
        a.use_gn = 1;
        return a;
    }
    // cond-only: M_b = scale * W_out . blockdiag(ctx_b^T), packed per sample next to W_res (null: attn_res is Identity) -- as bf16x3 planes (x3) or fp32 fragments
    void pack_mix_weights(const Dec& D, const float* wo, const float* wr, float* wmix, int co_n, int ck, int nch, int nb_pad, size_t per, bool x3) {
        Op op;
        op.name = "pack_mix_weights";
        const float scale = 1.0f / std::sqrt((float)D.d);
        const int BB = B, fea = D.fea, d = D.d;
        const float* ctx = D.ctx;
        op.flop = 2.0 * B * co_n * (double)fea * d;
        op.run = [wo, wr, ctx, wmix, BB, co_n, fea, d, scale, ck, nch, nb_pad, per, x3](hipStream_t s, const StepCtx&) {
            if (x3) hipLaunchKernelGGL(pack_mix_weights_x3_kernel, ew_grid(per * BB), dim3(256), 0, s, wo, wr, (const float*)ctx, BB, co_n, fea, d, scale, ck, nch, nb_pad, wmix);
            else hipLaunchKernelGGL(pack_mix_weights_kernel, ew_grid(per * BB), dim3(256), 0, s, wo, wr, (const float*)ctx, BB, co_n, fea, d, scale, ck, nch, nb_pad, wmix);
        };
        pre.push_back(std::move(op));
    }
    // train: f0 = ffn.0(a); f1 = silu(f0); f2 = ffn.2(f1); f3c = ffn.3(f2) + b   (every intermediate kept for the reverse pass)
    int ffn_train(const Dec& D, Tensor a, Tensor* f0, Tensor* f1, Tensor* f2, Tensor* f3c) {
        const int Hl = D.Hl, Wl = D.Wl;
        ConvSpec s;
        DDIF_TRY(need_conv(D.ci + ".ffn.0", &s.pc));
        s.in0 = a;
        s.use_bias = false;
        s.name = "ffn.0 (train)";
        DDIF_TRY(p.add_conv(step, s, f0));
        DDIF_TRY(p.alloc_tensor(f1, f0->C, f0->H, f0->W, true));
        Op op;
        op.name = "silu";
        op.cls = cls_small(Hl * Wl, 5);
        op.bytes = 8.0 * B * Hl * Wl * f0->C;
        Tensor ff0 = *f0, ff1 = *f1;
        const size_t n = (size_t)B * Hl * Wl * f0->C;
        op.run = [ff0, ff1, n](hipStream_t st, const StepCtx&) { tk::silu_fwd(st, ff0.p, n, ff1.p); };
        step.push_back(std::move(op));
        ConvSpec s2;
        DDIF_TRY(need_conv(D.ci + ".ffn.2", &s2.pc));
        s2.in0 = *f1;
        s2.use_bias = false;
        s2.name = "ffn.2 (train)";
        DDIF_TRY(p.add_conv(step, s2, f2));
        ConvSpec s3;
        DDIF_TRY(need_conv(D.ci + ".ffn.3", &s3.pc));
        s3.in0 = *f2;
        s3.name = "ffn.3 (train)";
        return p.add_conv(step, s3, f3c);
    }
    // train: out = a + ffn_drop_path(f3c)  (sr3_dwt.py:576): the per-sample DropPath scale sits between the conv and the residual
    int droppath_add(Tensor f3c, Tensor a, Tensor* out, float** scale_out) {
        Tensor f3;
        float* scale = nullptr;
        DDIF_TRY(p.alloc_tensor(&f3, f3c.C, f3c.H, f3c.W, true));
        DDIF_TRY(p.dalloc(&scale, (size_t)B));
        p.path_sites.push_back(scale);
        const int HW = f3c.H * f3c.W, Cc = f3c.C, BB = B;
        int chunks = (HW * Cc / 4 + 256 * 8 - 1) / (256 * 8);
        if (chunks < 1) chunks = 1;
        f3.np = chunks;
        DDIF_TRY(p.dalloc(&f3.st, (size_t)B * chunks * 2));
        Op op;
        op.name = "droppath_add";
        op.cls = cls_small(HW, 5);
        op.bytes = 12.0 * B * HW * Cc;
        op.run = [f3c, scale, a, f3, HW, Cc, BB, chunks](hipStream_t s, const StepCtx&) {
            hipLaunchKernelGGL(droppath_add_kernel, dim3(chunks, BB), dim3(256), 64, s, (const float*)f3c.p, (const float*)scale, (const float*)a.p, HW, Cc, f3.p, f3.st);
        };
        step.push_back(std::move(op));
        *out = f3;
        *scale_out = scale;
        return 0;
    }
    // ---- train mode: the block op by op (models/sr3_dwt.py:536-577), every intermediate the reverse pass needs kept in memory:
    //   xn = GN(cat[h, skip]), dwq = dw3x3(xn)        one launch (dw3x3_kernel, two sources, GroupNorm from the producers' partials)
    //   q = q.1(dwq);  o = linear attention(q, kv)     (kv comes from set_cond);  a = attn_out(o) + attn_res(xn)  as one 1x1 conv over cat[o, xn]
    //   f0 = ffn.0(a); f1 = silu(f0); f2 = ffn.2(f1); f3c = ffn.3(f2) + b;  out = a + DropPath(f3c)
    int decoder_block_train(const Dec& D, Tensor* out) {
        const std::string& ci = D.ci;
        const int BB = B, fea = D.fea, d = D.d, Hl = D.Hl, Wl = D.Wl;
        const PackedConv* pq1t = PC(ci + ".q.1");
        const PackedConv* pmixt = PC(ci + ".attn_mix");
        if (!pq1t || !pmixt) return fail(DDIF_ERR_MISSING, "%s: q.1 / attn_out missing", ci.c_str());
        if (!cur.st || !D.skip.st) return fail(DDIF_ERR_STATE, "%s: prenorm without producer statistics", ci.c_str());
        if (!D.pn_g || !D.pn_b || !D.q0w) return fail(DDIF_ERR_MISSING, "%s: prenorm/q.0 weights missing", ci.c_str());
        Tensor xn, dwq, q, o, a, f0, f1, f2, f3c, f3, kdw_pad;
        float *la_ctx = nullptr, *la_part = nullptr;
        DDIF_TRY(p.alloc_tensor(&xn, fea, Hl, Wl, true));
        DDIF_TRY(p.alloc_tensor(&dwq, fea, Hl, Wl, true));
        {
            DwArgs da = gn_dw_args(D, dwq, xn);
            da.tiles_x = (Wl + 15) / 16;
            da.tiles_y = (Hl + 7) / 8;
            Op op;
            op.name = "q.gn_dw3x3 (train)";
            op.cls = cls_small(Hl * Wl, 5);
            op.flop = 2.0 * 9 * B * Hl * Wl * fea;
            op.bytes = 12.0 * B * Hl * Wl * fea;
            op.run = [da](hipStream_t s, const StepCtx&) { launch_dw3x3(s, da); };
            step.push_back(std::move(op));
        }
        {
            ConvSpec s;
            s.pc = pq1t;
            s.in0 = dwq;
            s.name = "q.1x1 (train)";
            DDIF_TRY(p.add_conv(step, s, &q));
        }
        DDIF_TRY(p.alloc_tensor(&o, fea, Hl, Wl, true));
        {
            Op op;
            op.name = "linattn_fwd";
            op.cls = cls_small(Hl * Wl, 5);
            op.flop = 4.0 * B * 8 * d * d * (double)Hl * Wl;
            op.bytes = 16.0 * B * Hl * Wl * fea;
            Tensor qq = q, kk = D.kv, oo = o;
            if ((Hl > Wl ? Hl : Wl) * fea > 8192 || d > 32 || d % 4)
                return fail(DDIF_ERR_INVALID, "%s: train-mode linear attention holds one image line x %d channels in LDS: lines of more than %d pixels are not supported",
                            ci.c_str(), fea, 8192 / fea);
            DDIF_TRY(p.dalloc(&la_ctx, (size_t)B * fea * d));
            DDIF_TRY(p.dalloc(&la_part, tk::linattn_part_floats(B, Hl, Wl, fea, d)));
            float *cx = la_ctx, *pt = la_part;
            {   // cond-only half: softmax_W(k), context = k v^T per head (sr3_dwt.py:541,546,563) -- part of set_cond, like the eval plan's
                Op pc;
                pc.name = "linattn_ctx (train)";
                pc.bytes = 8.0 * B * Hl * Wl * fea;
                pc.run = [kk, BB, d, Hl, Wl, cx, pt](hipStream_t s, const StepCtx&) { tk::linattn_ctx(s, kk.p, BB, 8, d, Hl, Wl, cx, pt); };
                pre.push_back(std::move(pc));
                for (size_t i = D.pre_dec0; i < pre.size(); ++i) pre[i].side = true;
            }
            op.run = [qq, oo, BB, d, Hl, Wl, fea, cx](hipStream_t s, const StepCtx&) { tk::linattn_apply(s, qq.p, cx, BB, 8, d, Hl, Wl, oo.p, fea); };
            step.push_back(std::move(op));
        }
        const bool has_res = pmixt->cin == 2 * fea;
        {
            ConvSpec s;
            s.pc = pmixt;
            s.in0 = o;
            if (has_res) s.in1 = xn;
            else s.res = xn.p;  // attn_res is Identity
            s.name = "attn_out+res (train)";
            DDIF_TRY(p.add_conv(step, s, &a));
        }
        DDIF_TRY(ffn_train(D, a, &f0, &f1, &f2, &f3c));
        float* scale = nullptr;
        DDIF_TRY(droppath_add(f3c, a, &f3, &scale));
        // kv.0's output zero-padded to 4 | channels: input of kv.1's weight gradient (cond-only)
        DDIF_TRY(p.alloc_tensor(&kdw_pad, (D.cd + 3) & ~3, Hl, Wl));
        Plan::TrainMod& m = tmod(Plan::TrainMod::DEC, ci, cur, f3);
        m.t[0] = D.skip;
        m.t[1] = xn;
        m.t[2] = dwq;
        m.t[3] = q;
        m.t[4] = D.kv;
        m.t[5] = D.kdw;
        m.t[6] = kdw_pad;
        m.t[7] = o;
        m.t[8] = a;
        m.t[9] = f0;
        m.t[10] = f1;
        m.t[11] = f2;
        m.scale = scale;
        m.ctx = la_ctx;
        m.la_part = la_part;
        m.has_res = has_res;
        m.skip_from = D.skip_from;
        m.lev = lev;
        // f3c is only needed by the reverse pass through DropPath's scale: d(f3c) = scale * d(out); not stored in the record
        *out = f3;
        return 0;
    }
    // ---- inference: the whole attention half in ONE launch where the level keeps whole image columns inside a workgroup (kernels_lafuse.h):
    //      xn = GN(cat[h, skip]) -> q = q.1(q.0(xn)) -> softmax over H -> M_b p + W_res xn + bias; q and xn never reach memory.
    //      *fused = false: the level / shapes / weights do not admit it, nothing was emitted
    int linattn_fused(const Dec& D, const PackedConv* pq1, Tensor* amix, bool* fused) {
        const std::string& ci = D.ci;
        const int fea = D.fea, Hl = D.Hl, Wl = D.Wl;
        const Tensor& skip = D.skip;
        *fused = false;
        const PackedConv* pm = PC(ci + ".attn_mix");
        const float* wr = V(ci + ".attn_res.weight");
        // (round 6) the 8 x 8 level has a kernel of its own: half a sample per workgroup, the waves split the output channels (kernels_lafuse8.h)
        const bool la8 = la8_enabled() && lafuse8_supported(Hl, Wl, cur.C, skip.C, pm ? pm->cout : 0);
        bool ok = lafuse_enabled() && f16_enabled() && x3_enabled() && lr_enabled() && pm && wr && pq1->w_f16 && pq1->bias && pm->bias && (Hl * Wl >= 256 || la8) &&
                  pq1->cout == fea && pq1->ck == 32 && pm->ck == 32 && pm->cin == 2 * fea && cur.C % 16 == 0 && skip.C % 16 == 0 && (la8 || lafuse_supported(Hl, fea, pm->cout));
        if (ok) {  // f16x2 range of depthwise(GroupNorm(.)): (sqrt(N) max|gamma| + max|beta|) * 9 max|w_dw| inside the scaled half range
            auto ig = net.vec_absmax.find(D.pn_g), ib = net.vec_absmax.find(D.pn_b), iw = net.vec_absmax.find(D.q0w);
            ok = ig != net.vec_absmax.end() && ib != net.vec_absmax.end() && iw != net.vec_absmax.end() &&
                 (std::sqrt((double)fea * Hl * Wl) * ig->second + ib->second) * 9.0 * iw->second < DDIF_F16_AMAX;
        }
        if (!ok) return 0;
        const float* wo = V(ci + ".attn_out.weight");
        if (!wo) return fail(DDIF_ERR_MISSING, "%s.attn_out.weight missing", ci.c_str());
        const int nb_pad = (((pm->cout + 31) / 32) + 3) & ~3;
        const size_t per = (size_t)nb_pad * pm->n_chunks * 2 * 3 * 256;  // bf16x3 planes, 32-channel chunks
        float* wmix = nullptr;
        DDIF_TRY(p.dalloc(&wmix, per * B));
        pack_mix_weights(D, wo, wr, wmix, pm->cout, 32, pm->n_chunks, nb_pad, per, true);
        p.use(cur.p);
        p.use(skip.p);
        DDIF_TRY(p.alloc_tensor(amix, pm->cout, Hl, Wl, true));
        LaFuseArgs a{};
        a.xcd = (xcd_mask() & 4) ? 1 : 0;
        a.in0 = cur.p;
        a.c0 = cur.C;
        a.in1 = skip.p;
        a.c1 = skip.C;
        a.B = B;
        a.H = Hl;
        a.W = Wl;
        a.st0 = cur.st;
        a.np0 = cur.np;
        a.st1 = skip.st;
        a.np1 = skip.np;
        a.gamma = D.pn_g;
        a.beta = D.pn_b;
        a.dw_w = D.q0w;
        a.wq = pq1->w_f16;
        a.nchq = pq1->n_chunks;
        a.bq = pq1->bias;
        a.wmix = wmix;
        a.wmix_bstride = (long long)per;
        a.nch_mix = pm->n_chunks;
        a.bias = pm->bias;
        a.out = amix->p;
        a.dout = pm->cout;
        {   // attn_res(xn) on f16x2 (three products, two operand planes) under the rule of attn_block's qkv: W_res has a half pack (|w| < 64, ddif_net.cpp) and the
            // bound sqrt(N) max|gamma| + max|beta| of prenorm_x's output stays inside the scaled half range; otherwise, and under DDIF_LA_RES_F16=0, bf16x3 out of
            // the per-sample [M_b | W_res] pack, whose size and layout do not depend on the choice
            static const bool rf16 = env_flag("DDIF_LA_RES_F16", true);
            const float* w16 = V(ci + ".attn_res.weight.f16");
            auto ig = net.vec_absmax.find(D.pn_g), ib = net.vec_absmax.find(D.pn_b);
            const bool okr = ig != net.vec_absmax.end() && ib != net.vec_absmax.end() &&
                             std::sqrt((double)fea * Hl * Wl) * ig->second + ib->second < DDIF_F16_AMAX;
            a.wres16 = (rf16 && w16 && okr) ? w16 : nullptr;
            a.nchr = fea / 32;
        }
        // four-wave workgroups of 128 pixels instead of eight-wave ones of 256 when the latter would not fill the CUs (round 6; same results either way:
        // kernels_lafuse.h).  DDIF_LA_NW = 8 / 4 forces one form (tests/test_env_switches.py).
        int la_nw = 8;
        if (!la8) {
            static const int nw_env = env_int("DDIF_LA_NW", 0);
            const long wg8 = (long)B * ((Wl + lafuse_strip(Hl, 8) - 1) / lafuse_strip(Hl, 8));
            la_nw = nw_env == 4 || nw_env == 8 ? nw_env : (wg8 < num_cus() ? 4 : 8);
        }
        // ... and 64-pixel workgroups whose four waves split the output channels (kernels_lafuse.h CS = 2) when twice the four-wave grid still fits the CUs (the 16 x 16
        // level up to B = 64 on 256 CUs); never where the four-wave grid already fills them.  Bit-identical either way; DDIF_LA_CSPLIT=0 keeps the four-wave form
        int la_cs = 1;
        if (!la8 && la_nw == 4) {
            static const bool cs_env = env_flag("DDIF_LA_CSPLIT", true);
            const long wg4 = (long)B * ((Wl + lafuse_strip(Hl, 4) - 1) / lafuse_strip(Hl, 4));
            if (cs_env && lafuse_csplit_supported(Hl, fea, pm->cout) && 2 * wg4 <= num_cus()) la_cs = 2;
        }
        if (!p.dry) DDIF_TRY(la8 ? lafuse8_launch(a, 1, nullptr, true) : lafuse_launch(a, 1, nullptr, true, la_nw, la_cs));
        const int nstrips = la8 ? 2 : (Wl + lafuse_strip(Hl, la_nw, la_cs) - 1) / lafuse_strip(Hl, la_nw, la_cs);
        long cap = num_cus();
        if (g_debug_grid_cap > 0 && g_debug_grid_cap < cap) cap = g_debug_grid_cap;
        Op op;
        op.name = la8 ? "linattn8_fused" : "linattn_fused";
        {
            char lb[160];
            snprintf(lb, sizeof lb, "linattn_fused GN+dw3x3+q.1+softmax_H+attn_out+res(%s) %d+%d->%d @%dx%d", a.wres16 ? "f16x2" : "bf16x3", cur.C, skip.C, pm->cout, Hl, Wl);
            op.label = lb;
        }
        if (getenv("DDIF_DUMP_PLAN"))  // (its own prefix: the `[ddif plan]` lines are the convs of add_conv, tools/plan_signature.py)
            fprintf(stderr, "[ddif la] %-34s res=%s nw=%d csplit=%d\n", ci.c_str(), a.wres16 ? "f16x2" : "bf16x3", la_nw, la_cs);
        op.flop = 2.0 * B * Hl * Wl * ((double)fea * fea + 9.0 * fea + 2.0 * fea * pm->cout);
        op.bytes = 4.0 * B * Hl * Wl * ((double)fea + pm->cout);
        op.cls = cls_small(Hl * Wl, 1);
        // q.1 on f16x2 (x3), attn_out on bf16x3 (x6), attn_res on either: weight of the sum
        op.mfma_w = (3.0 * fea * fea + (6.0 + (a.wres16 ? 3.0 : 6.0)) * fea * pm->cout) / ((double)fea * fea + 9.0 * fea + 2.0 * fea * pm->cout);
        op.run = [a, nstrips, cap, la8, la_nw, la_cs](hipStream_t st, const StepCtx&) {
            const long nw = (long)a.B * nstrips;
            if (la8) (void)lafuse8_launch(a, (int)(nw < cap ? nw : cap), st, false);
            else (void)lafuse_launch(a, (int)(nw < cap ? nw : cap), st, false, la_nw, la_cs);
        };
        step.push_back(std::move(op));
        *fused = true;
        return 0;
    }
    // low-resolution levels: xn = GN(cat), dwq = depthwise3x3(xn) from ONE small kernel (whole sample per workgroup), then q = q.1(dwq) on the split-K
    // kernel -- fused into the 1x1 conv the depthwise pass would be recomputed by every 32-cout tile (sr3_dwt.py:507-513,537,540)
    int q_low_resolution(const Dec& D, const PackedConv* pq1, Tensor xn, Tensor* q, float** qmx, float** qsm) {
        const int BB = B, fea = D.fea, Hl = D.Hl, Wl = D.Wl;
        Tensor dwq;
        DDIF_TRY(p.alloc_tensor(&dwq, fea, Hl, Wl, true));
        p.use(cur.p);
        p.use(D.skip.p);
        p.use(xn.p);
        DwArgs a = gn_dw_args(D, dwq, xn);
        Op op;
        op.name = "q.gn_dw3x3";
        op.cls = 2;
        {
            char lb[160];
            snprintf(lb, sizeof lb, "q.gn_dw3x3 %d+%d @%dx%d", cur.C, D.skip.C, Hl, Wl);
            op.label = lb;
        }
        op.flop = 2.0 * 9 * B * Hl * Wl * fea;
        op.bytes = 4.0 * B * Hl * Wl * 3.0 * fea;
        const size_t sm = (size_t)(Hl + 2) * (Wl + 2) * 36 * sizeof(float);
        if (sm > 64 * 1024) DDIF_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(gn_dw3x3_small_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
        a.xcd = (xcd_mask() & 8) ? 1 : 0;
        const dim3 gdw = a.xcd ? dim3(BB, (fea + 31) / 32) : dim3((fea + 31) / 32, BB);
        op.run = [a, gdw, sm](hipStream_t s, const StepCtx&) { hipLaunchKernelGGL(gn_dw3x3_small_kernel, gdw, dim3(256), sm, s, a); };
        step.push_back(std::move(op));
        ConvSpec s;
        s.pc = pq1;
        s.in0 = dwq;
        s.name = "q.1x1";
        if (Hl <= 16) {  // whole columns inside one tile: softmax_H statistics of q from the conv's epilogue
            DDIF_TRY(p.dalloc(qmx, (size_t)B * Wl * fea));
            DDIF_TRY(p.dalloc(qsm, (size_t)B * Wl * fea));
            s.cso_mx = *qmx;
            s.cso_sm = *qsm;
            s.name = "q.1x1 (+softmax_H stats)";
        }
        return p.add_conv(step, s, q);
    }
    // inference, where the fused block does not apply: q conv (-> xn, q), column statistics of q, attn_out conv on per-sample weights
    int linattn_three_launch(const Dec& D, const PackedConv* pq1, Tensor* amix) {
        const std::string& ci = D.ci;
        const int BB = B, fea = D.fea, Hl = D.Hl, Wl = D.Wl;
        const Tensor& skip = D.skip;
        Tensor xn, q;
        DDIF_TRY(p.alloc_tensor(&xn, fea, Hl, Wl, true));
        if (pq1->ck != 32 || cur.C % 4 != 0 || skip.C % 4 != 0 || fea > 256)
            return fail(DDIF_ERR_INVALID, "%s: the fused q = 1x1(dw3x3(GN(cat))) kernel needs 4 | channels and <= 256 of them (got %d+%d)", ci.c_str(), cur.C, skip.C);
        float *qmx = nullptr, *qsm = nullptr;
        if (pick_cfg(CfgQuery{1, 32, PRO_NONE, 1, 1, 0, Hl, Wl, pq1->cout, B, fea, fea}) >= 20) {
            DDIF_TRY(q_low_resolution(D, pq1, xn, &q, &qmx, &qsm));
        } else {
            // q = q.1(depthwise3x3(GroupNorm(cat[h, skip]))) in ONE kernel; also emits xn (sr3_dwt.py:507-513,537,540)
            ConvSpec s;
            s.pc = pq1;
            s.in0 = cur;
            s.in1 = skip;
            s.pro = PRO_GN_DW;
            s.gamma = D.pn_g;
            s.beta = D.pn_b;
            s.dw_w = D.q0w;
            s.out_xn = xn.p;
            s.name = "q = 1x1(dw3x3(GN(cat)))";
            DDIF_TRY(p.add_conv(step, s, &q));
        }
        if (!qmx) {
            DDIF_TRY(p.dalloc(&qmx, (size_t)B * Wl * fea));
            DDIF_TRY(p.dalloc(&qsm, (size_t)B * Wl * fea));
            p.use(q.p);
            Op op;
            op.name = "q.softmax_stats";
            op.cls = 4;
            op.bytes = 8.0 * B * Hl * Wl * fea;
            op.run = [q, qmx, qsm, fea, BB, Hl, Wl](hipStream_t s, const StepCtx&) {
                hipLaunchKernelGGL(softmax_stats_kernel, ew_grid((size_t)BB * Wl * fea), dim3(256), 0, s, (const float*)q.p, fea, 0, fea, BB, Hl, Wl, 0, qmx, qsm);
            };
            step.push_back(std::move(op));
        }
        const PackedConv* pmix = PC(ci + ".attn_mix");
        if (!pmix) return fail(DDIF_ERR_MISSING, "%s.attn_out missing", ci.c_str());
        // the linear-attention context is folded into per-sample attn_out weights (needs 32-channel chunks)
        if (fea % 32 != 0 || pmix->ck != 32) return fail(DDIF_ERR_INVALID, "%s: linear attention over %d channels needs 32 | channels", ci.c_str(), fea);
        const int nb_pad = (((pmix->cout + 31) / 32) + 3) & ~3;
        // the layout follows the instantiation add_conv() will pick for this conv (bf16x3 planes or fp32 fragments)
        const bool mix_x3 = pick_cfg(CfgQuery{1, pmix->ck, PRO_COLSM, 1, 1, 0, Hl, Wl, pmix->cout, B, pmix->cin, pmix->cin == 2 * fea ? fea : pmix->cin}) >= 12;
        const size_t per = mix_x3 ? (size_t)nb_pad * pmix->n_chunks * (pmix->ck / 16) * 3 * 256 : (size_t)nb_pad * pmix->n_chunks * (pmix->ck / 8) * 256;
        float* wmix = nullptr;
        DDIF_TRY(p.dalloc(&wmix, per * B));
        const float* wo = V(ci + ".attn_out.weight");
        const float* wr = V(ci + ".attn_res.weight");  // null: attn_res is Identity
        if (!wo) return fail(DDIF_ERR_MISSING, "%s.attn_out.weight missing", ci.c_str());
        pack_mix_weights(D, wo, wr, wmix, pmix->cout, pmix->ck, pmix->n_chunks, nb_pad, per, mix_x3);
        ConvSpec s;
        s.pc = pmix;
        s.in0 = q;
        if (pmix->cin == 2 * fea) s.in1 = xn;
        else s.res = xn.p;  // attn_res is Identity
        s.pro = PRO_COLSM;
        s.cs_mx = qmx;
        s.cs_sm = qsm;
        s.w_override = wmix;
        s.w_bstride = (long long)per;
        s.name = "softmax_H(q).ctx.attn_out+res";
        return p.add_conv(step, s, amix);
    }
    // inference: f1 = silu(ffn.0(a)), then ffn[3] o ffn[2] as ONE 3x3 conv where the net carries the merged weights ".ffn.23" (no nonlinearity between
    // them; ddif_net.cpp), else as two convs; the residual a rides in the last conv's epilogue.  (The train-mode decoder has its own: ffn_train.)
    int ffn(const Dec& D, Tensor amix, Tensor* f3) {
        Tensor f1, f2;
        ConvSpec s;
        DDIF_TRY(need_conv(D.ci + ".ffn.0", &s.pc));
        s.in0 = amix;
        s.use_bias = false;
        s.silu = true;
        s.name = "ffn.0";
        DDIF_TRY(p.add_conv(step, s, &f1));
        ConvSpec s2;
        DDIF_TRY(need_conv(D.ci + ".ffn.2", &s2.pc));
        s2.in0 = f1;
        s2.use_bias = false;
        s2.name = "ffn.2";
        ConvSpec s3;
        DDIF_TRY(need_conv(D.ci + ".ffn.3", &s3.pc));
        if (const PackedConv* pm = PC(D.ci + ".ffn.23")) {
            ConvSpec sf = s2;
            sf.pc = pm;
            sf.use_bias = true;
            sf.res = amix.p;
            sf.stats = true;
            sf.name = "ffn.3(ffn.2) merged + res";
            return p.add_conv(step, sf, f3);
        }
        DDIF_TRY(p.add_conv(step, s2, &f2));
        s3.in0 = f2;
        s3.res = amix.p;
        s3.stats = true;
        s3.name = "ffn.3";
        return p.add_conv(step, s3, f3);
    }
    // FastAttnCondInjection (sr3_dwt.py:495-577) + ResnetBlocWithAttn
    int decoder_block(const Layer& L) {
        Dec D;
        D.ci = L.p + ".cond_inj";
        D.skip = feats.back();
        feats.pop_back();
        if (train) {
            D.skip_from = feat_mod.back();
            feat_mod.pop_back();
        }
        if (D.skip.C != L.cskip || cur.C != L.cx || D.skip.H != cur.H || D.skip.W != cur.W)
            return fail(DDIF_ERR_INVALID, "%s: skip/feature shape mismatch", L.p.c_str());
        D.fea = L.cin;
        D.d = D.fea / 8;
        D.Hl = cur.H;
        D.Wl = cur.W;
        D.cd = Cl + 3 * Pn;
        DDIF_TRY(decoder_context(D));
        const std::string& ci = D.ci;
        D.pn_g = V(ci + ".prenorm_x.weight");
        D.pn_b = V(ci + ".prenorm_x.bias");
        D.q0w = V(ci + ".q.0.weight");
        Tensor f3;
        if (train) {
            DDIF_TRY(decoder_block_train(D, &f3));
        } else {
            // ---- per step
            const PackedConv* pq1 = PC(ci + ".q.1");
            if (!pq1) return fail(DDIF_ERR_MISSING, "%s.q.1 missing", ci.c_str());
            if (!cur.st || !D.skip.st) return fail(DDIF_ERR_STATE, "%s: prenorm without producer statistics", ci.c_str());
            if (!D.pn_g || !D.pn_b || !D.q0w) return fail(DDIF_ERR_MISSING, "%s: prenorm/q.0 weights missing", ci.c_str());
            p.tap(ci + ".cur", cur);
            p.tap(ci + ".skip", D.skip);
            p.tap(ci + ".cond", p.cdec[lev], true);
            Tensor amix;
            bool fused_attn = false;
            DDIF_TRY(linattn_fused(D, pq1, &amix, &fused_attn));
            if (!fused_attn) DDIF_TRY(linattn_three_launch(D, pq1, &amix));
            p.tap(ci + ".a", amix);
            DDIF_TRY(ffn(D, amix, &f3));
            p.tap(ci + ".out", f3);
        }
        DDIF_TRY(resblock(L.p + ".res_block", f3, &cur));
        return attention_if(L);
    }
    int final_conv() {
        ConvSpec s;
        DDIF_TRY(need_conv("final_conv.block.3", &s.pc));
        s.in0 = cur;
        s.pro = PRO_GN_SILU;
        s.gamma = V("final_conv.block.0.weight");
        s.beta = V("final_conv.block.0.bias");
        s.name = "final";
        s.samp = true;
        DDIF_TRY(p.add_conv(step, s, &p.net_out));
        if (train) tmod(Plan::TrainMod::FINAL, "final_conv", cur, p.net_out);
        return 0;
    }
};
}  // namespace

// UNetSR3.forward (reference models/sr3_dwt.py:169-219) as a launch program, the cond-only branches hoisted into set_cond
int Plan::build_impl() {
    const ddif_net_cfg& c = net->cfg;
    if (!net->committed) return fail(DDIF_ERR_STATE, "ddif_plan_create: ddif_net_commit has not been called");
    C = c.out_channel;
    P = c.pan_channel;
    CC = 2 * c.lms_channel + 4 * P;
    const int nlev = c.n_channel_mults;
    const int div = 1 << (nlev - 1);
    if (B < 1 || H < div || W < div || H % div || W % div)
        return fail(DDIF_ERR_INVALID, "ddif_plan_create: H=%d W=%d must be positive multiples of %d", H, W, div);
    LH.assign(1, H);
    LW.assign(1, W);
    for (int l = 1; l < nlev; ++l) {
        LH.push_back((LH.back() - 1) / 2 + 1);
        LW.push_back((LW.back() - 1) / 2 + 1);
    }
    PlanBuilder b(*this);
    DDIF_TRY(b.boundary_buffers());
    DDIF_TRY(b.cond_program());
    for (size_t li = 0; li < net->downs.size(); ++li) {
        const Layer& L = net->downs[li];
        DDIF_TRY(L.kind == L_STEM ? b.stem(li) : (L.kind == L_DOWN ? b.down(li) : b.encoder_block(li)));
        tap(L.p, b.cur);
        b.feats.push_back(b.cur);
        if (train_mode) {
            tmods.back().pushes_feat = true;
            b.feat_mod.push_back((int)tmods.size() - 1);
        }
    }
    for (const Layer& L : net->mid) {
        DDIF_TRY(b.mid_block(L));
        tap(L.p, b.cur);
    }
    if (train_mode) b.join_side_stream();
    for (const Layer& L : net->ups) {
        DDIF_TRY(L.kind == L_UP ? b.up(L) : b.decoder_block(L));
        tap(L.p, b.cur);
    }
    DDIF_TRY(b.final_conv());
    DDIF_TRY(ensure_tb(B));
    return 0;
}
#undef DDIF_TRY

void Plan::drop_graphs() {
#ifndef DDIF_EMU
    for (auto& g : graph_exec) {
        if (g) (void)hipGraphExecDestroy((hipGraphExec_t)g);
        g = nullptr;
    }
#endif
}

int Plan::ensure_tb(int rows) {
    if (rows <= tb_rows) return 0;
    drop_graphs();  // captured launches point at the old table
    if (int e = dalloc(&tb, (size_t)rows * net->nslots)) return e;  // older table stays in `allocs` until destroy
    if (int e = dalloc(&tvals, (size_t)rows)) return e;
    tb_rows = rows;
    return 0;
}

int Plan::time_rows(const float* t_host, int rows, hipStream_t s) { return time_rows_aux(t_host, rows, nullptr, s); }

static int check_sampler_net(const Net* n);

int Plan::time_rows_aux(const float* t_host, int rows, float* aux, hipStream_t s) {
    if (int e = ensure_tb(rows)) return e;
    DDIF_HIPCHK(hipMemcpyAsync(tvals, t_host, (size_t)rows * sizeof(float), hipMemcpyDefault, s));  // host or device source
    const int inner = net->cfg.inner_channel;
    hipLaunchKernelGGL(time_embed_kernel, dim3(rows), dim3(128), (size_t)6 * inner * sizeof(float), s, (const float*)tvals,
                       net->freqs, net->w1, net->b1, net->w3, net->b3, net->wall, net->ball, inner, net->nslots, tb, aux);
    return 0;
}

namespace tk {
void dw3x3_plain(hipStream_t s, const float* in, int C, int B, int H, int W, const float* w9c, float* out, bool flip) {
    DwArgs a{};
    a.flip = flip ? 1 : 0;
    a.in0 = in;
    a.c0 = C;
    a.B = B;
    a.H = H;
    a.W = W;
    a.w = w9c;
    a.out_dw = out;
    a.tiles_x = (W + 15) / 16;
    a.tiles_y = (H + 7) / 8;
    launch_dw3x3(s, a);
}
}  // namespace tk

// One training iteration's device work (reference diffusion_ddpm_pan.py:692-766 main pass + diffusion_engine.py:233 loss.backward()):
// x_t = a x0 + s noise, train-mode forward (masks as set), L1 loss against x0, reverse program -> gradients in the bound tensors.
int Plan::train_step(const float* x0, const float* noise, const float* a_h, const float* s_h, const float* t_h, const float* sc, float* loss_dev, float* pred,
                     hipStream_t s, const ddif_objective_rows* rows, float* recon_out) {
    if (!train_mode || bwd.empty()) return fail(DDIF_ERR_STATE, "ddif_plan_train_step: not a train-mode plan");
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_train_step before ddif_plan_set_cond");
    if (!x0 || !noise || !a_h || !s_h || !t_h) return fail(DDIF_ERR_INVALID, "ddif_plan_train_step: NULL argument");
    for (auto& kv : grad_slots)
        if (!kv.second) return fail(DDIF_ERR_STATE, "ddif_plan_train_step: gradient tensors are not bound (ddif_plan_train_bind); first missing: %s", kv.first.c_str());
    if (int e = check_sampler_net(net)) return e;
    const int HW = H * W;
    const size_t n = (size_t)B * HW * C;
    DDIF_HIPCHK(hipMemcpyAsync(small, a_h, (size_t)B * sizeof(float), hipMemcpyDefault, s));  // host or device source
    DDIF_HIPCHK(hipMemcpyAsync(small + B, s_h, (size_t)B * sizeof(float), hipMemcpyDefault, s));
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, x0, B, C, HW, 0, C, img[0]);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, noise, B, C, HW, 0, C, img[1]);
    const bool p2 = rows && rows->p2_weight;
    if (pred_mode != DDIF_PRED_X_START || p2 || recon_out)
        if (int e = objective_rows(rows, p2, s)) return e;
    const float* target = img[0];  // x_start (:729-732)
    if (pred_mode == DDIF_PRED_V) {  // v = a noise - s x0 (:734), written by the pass that writes x_t
        if (!vtarget)
            if (int e = dalloc(&vtarget, n)) return e;
        hipLaunchKernelGGL(q_sample_v_kernel, ew_grid(n), dim3(256), 0, s, (const float*)img[0], (const float*)img[1], (const float*)small, (const float*)(small + B), B, (size_t)HW * C, x_in.p, vtarget);
        target = vtarget;
    } else {
        hipLaunchKernelGGL(q_sample_kernel, ew_grid(n), dim3(256), 0, s, (const float*)img[0], (const float*)img[1], (const float*)small, (const float*)(small + B), B, (size_t)HW * C, x_in.p);
        if (pred_mode == DDIF_PRED_NOISE) target = img[1];  // the noise itself (:726-728)
    }
    if (sc) hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, sc, B, C, HW, 0, C, sc_in.p);
    if (int e = train_core(t_h, sc != nullptr, target, loss_dev, pred, s, p2 ? obj_rows + 2 * (size_t)B : nullptr)) return e;
    if (recon_out) {
        // recon_x0 (:724, :730, :735): the reference rebuilds it from the prediction for noise and from the TRUE v for pred_v
        if (pred_mode == DDIF_PRED_X_START) hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)net_out.p, B, C, HW, recon_out);
        else if (int e = recon(pred_mode == DDIF_PRED_V ? vtarget : net_out.p, recon_out, true, s)) return e;
        DDIF_HIPCHK(hipGetLastError());
    }
    return 0;
}

// ---- objective (include/ddif.h ddif_plan_set_objective)
int Plan::set_objective(int pred, int loss) {
    if (pred != DDIF_PRED_X_START && pred != DDIF_PRED_NOISE && pred != DDIF_PRED_V) return fail(DDIF_ERR_INVALID, "ddif_plan_set_objective: pred_mode %d (0 x_start, 1 noise, 2 pred_v)", pred);
    if (loss != DDIF_LOSS_L1 && loss != DDIF_LOSS_L2 && loss != DDIF_LOSS_L1SSIM) return fail(DDIF_ERR_INVALID, "ddif_plan_set_objective: loss_type %d (0 l1, 1 l2, 2 l1ssim)", loss);
    if (loss == DDIF_LOSS_L1SSIM && train_mode && !ssim_maps) {  // the scratch of the SSIM tail (ddif_ssimloss.cpp): only a plan that trains under this loss pays for it
        if (int e = tk::ssimloss_check("ddif_plan_set_objective (l1ssim)", B, C, H, W)) return e;
        if (!ssim_part)
            if (int e = dalloc(&ssim_part, 2 * tk::ssimloss_workgroups(B, C, H, W))) return e;
        if (int e = dalloc(&ssim_maps, (size_t)3 * B * H * W * C)) return e;
    }
    if ((pred != DDIF_PRED_X_START) != (pred_mode != DDIF_PRED_X_START)) drop_graphs();  // the captured step holds the other final-conv instantiation
    pred_mode = pred;
    loss_type = loss;
    return 0;
}
// ---- dynamic thresholding (include/ddif.h ddif_plan_set_threshold)
int Plan::set_threshold(int mode, float ratio, float max_val) {
    if (mode != DDIF_THRESHOLD_OFF && mode != DDIF_THRESHOLD_DDPM && mode != DDIF_THRESHOLD_SOLVER)
        return fail(DDIF_ERR_INVALID, "ddif_plan_set_threshold: mode %d (0 off, 1 DDPM form, 2 solver form)", mode);
    if (mode != DDIF_THRESHOLD_OFF) {
        if (!(ratio >= 0.f && ratio <= 1.f)) return fail(DDIF_ERR_INVALID, "ddif_plan_set_threshold: ratio %g outside [0, 1]", (double)ratio);
        if (!(max_val >= 0.f) || max_val > 3.0e38f) return fail(DDIF_ERR_INVALID, "ddif_plan_set_threshold: max_val %g must be finite and >= 0", (double)max_val);
        if ((long long)H * W * C > 0x7fffffffLL) return fail(DDIF_ERR_INVALID, "ddif_plan_set_threshold: more than 2^31 values per sample");
        if (int e = quantile_prepare()) return e;
        if (!d_thr)
            if (int e = dalloc(&d_thr, (size_t)B)) return e;
    } else {
        ratio = 0.f;
        max_val = 1.f;
    }
    if (mode != thr_mode || ratio != thr_ratio || max_val != thr_max) drop_graphs();  // the captured pair holds the other tail / the old rank and floor
    thr_mode = mode;
    thr_ratio = ratio;
    thr_max = max_val;
    return 0;
}
// ---- overlapping tiles (include/ddif.h ddif_plan_set_tiling)
int Plan::set_tiling(const ddif_tiling* t) {
    if (!t) {
        if (tiling_on) drop_graphs();  // the captured pair holds the tiled tail
        tiling_on = false;
        return 0;
    }
    if (t->n_scenes < 1) return fail(DDIF_ERR_INVALID, "ddif_plan_set_tiling: n_scenes %d must be >= 1", t->n_scenes);
    if (t->overlap < 0 || t->overlap >= std::min(H, W)) return fail(DDIF_ERR_INVALID, "ddif_plan_set_tiling: overlap %d outside [0, min(H, W) = %d)", t->overlap, std::min(H, W));
    if (t->scene_h < H || t->scene_w < W) return fail(DDIF_ERR_INVALID, "ddif_plan_set_tiling: a scene of %dx%d is smaller than the plan's %dx%d tile", t->scene_h, t->scene_w, H, W);
    const int ny = ddif_tile_count(t->scene_h, H, t->overlap), nx = ddif_tile_count(t->scene_w, W, t->overlap);
    if ((long long)t->n_scenes * ny * nx != B)
        return fail(DDIF_ERR_INVALID, "ddif_plan_set_tiling: %d scenes of %dx%d in %dx%d tiles with overlap %d are %d x %d x %d tiles, the plan's batch is %d", t->n_scenes, t->scene_h,
                    t->scene_w, H, W, t->overlap, t->n_scenes, ny, nx, B);
    if (ny > 0x7fff || nx > 0x7fff || (long long)t->scene_h * t->scene_w > 0x7fffffffLL) return fail(DDIF_ERR_INVALID, "ddif_plan_set_tiling: the scene is too large for the tile table");
    const bool same_geom = ttab.tab && tiling.n_scenes == t->n_scenes && tiling.scene_h == t->scene_h && tiling.scene_w == t->scene_w && tiling.overlap == t->overlap;
    if (same_geom && tiling_on) return 0;
    if (!same_geom) {
        // py | px | ycov | xcov | mpx (tiling_args.h TileTab)
        std::vector<int> tab;
        for (int k = 0; k < ny; ++k) tab.push_back(ddif_tile_origin(k, t->scene_h, H, t->overlap));
        for (int k = 0; k < nx; ++k) tab.push_back(ddif_tile_origin(k, t->scene_w, W, t->overlap));
        auto covers = [&](int L, int tl, int n, int off) {
            for (int y = 0; y < L; ++y) {
                int first = 0, cnt = 0;
                for (int k = 0; k < n; ++k)
                    if (tab[off + k] <= y && y < tab[off + k] + tl) {
                        if (!cnt) first = k;
                        ++cnt;
                    }
                tab.push_back(first | (cnt << 16));
            }
        };
        covers(t->scene_h, H, ny, 0);
        covers(t->scene_w, W, nx, ny);
        const int* ycov = tab.data() + ny + nx;
        int npx = 0;
        for (int y = 0; y < t->scene_h; ++y)
            for (int x = 0; x < t->scene_w; ++x)
                if ((ycov[y] >> 16) * (ycov[t->scene_h + x] >> 16) > 1) ++npx;
        tab.reserve(tab.size() + npx);
        for (int y = 0; y < t->scene_h; ++y)
            for (int x = 0; x < t->scene_w; ++x) {
                const int cy = tab[ny + nx + y] >> 16, cx = tab[ny + nx + t->scene_h + x] >> 16;
                if (cy * cx > 1) tab.push_back(y * t->scene_w + x);
            }
        int* d = nullptr;
        if (int e = dalloc(&d, tab.size())) return e;  // a new table: work in flight may still read the old one, which stays in `allocs` until destroy
        DDIF_HIPCHK(hipMemcpy(d, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
        ttab = TileTab{d, t->n_scenes, t->scene_h, t->scene_w, H, W, ny, nx, npx};
        tiling = *t;
    }
    drop_graphs();  // the captured pair holds the other tail / the other table
    tiling_on = true;
    return 0;
}
// device copies of the caller's per-sample rows (host or device source, like sqrt_ac / sqrt_1mac)
int Plan::objective_rows(const ddif_objective_rows* rows, bool need_p2, hipStream_t s) {
    const bool need_rec = pred_mode != DDIF_PRED_X_START;
    if ((need_rec || need_p2) && !rows) return fail(DDIF_ERR_INVALID, "the plan's objective needs ddif_objective_rows");
    if (need_rec && (!rows->recon_xt || !rows->recon_out)) return fail(DDIF_ERR_INVALID, "ddif_objective_rows: recon_xt / recon_out are required for a noise / v prediction");
    if (!obj_rows)
        if (int e = dalloc(&obj_rows, (size_t)3 * B)) return e;
    if (need_rec) {
        DDIF_HIPCHK(hipMemcpyAsync(obj_rows, rows->recon_xt, (size_t)B * sizeof(float), hipMemcpyDefault, s));
        DDIF_HIPCHK(hipMemcpyAsync(obj_rows + B, rows->recon_out, (size_t)B * sizeof(float), hipMemcpyDefault, s));
    }
    if (need_p2) DDIF_HIPCHK(hipMemcpyAsync(obj_rows + 2 * (size_t)B, rows->p2_weight, (size_t)B * sizeof(float), hipMemcpyDefault, s));
    return 0;
}
int Plan::recon(const float* src_nhwc, float* out, bool nchw, hipStream_t s) {
    const int HW = H * W;
    hipLaunchKernelGGL(recon_x0_kernel, ew_grid((size_t)B * HW * C), dim3(256), 0, s, (const float*)x_in.p, src_nhwc, (const float*)obj_rows, (const float*)(obj_rows + B), B, C, HW,
                       nchw ? 1 : 0, out);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

// forward + loss + reverse pass on a GIVEN network input (parity tests feed the reference's own x / target): x, target (B,C,H,W)
int Plan::train_forward_backward(const float* x, const float* t_h, const float* sc, const float* target, float* loss_dev, float* pred, hipStream_t s) {
    if (!train_mode || bwd.empty()) return fail(DDIF_ERR_STATE, "ddif_plan_train_forward_backward: not a train-mode plan");
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_train_forward_backward before ddif_plan_set_cond");
    if (!x || !t_h || !target) return fail(DDIF_ERR_INVALID, "ddif_plan_train_forward_backward: NULL argument");
    for (auto& kv : grad_slots)
        if (!kv.second) return fail(DDIF_ERR_STATE, "ddif_plan_train_forward_backward: gradient tensors are not bound; first missing: %s", kv.first.c_str());
    if (int e = check_sampler_net(net)) return e;
    const int HW = H * W;
    const size_t n = (size_t)B * HW * C;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, x, B, C, HW, 0, C, x_in.p);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, target, B, C, HW, 0, C, img[0]);
    if (sc) hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, sc, B, C, HW, 0, C, sc_in.p);
    return train_core(t_h, sc != nullptr, img[0], loss_dev, pred, s);
}

int Plan::train_core(const float* t_h, bool has_sc, const float* target_nhwc, float* loss_dev, float* pred, hipStream_t s, const float* p2w) {
    const int HW = H * W;
    const size_t n = (size_t)B * HW * C;
    if (int e = time_rows_aux(t_h, B, taux, s)) return e;
    StepCtx ctx;
    ctx.x = x_in.p;
    ctx.sc = has_sc ? sc_in.p : x_in.p;
    ctx.tb = tb;
    ctx.tb_stride = net->nslots;
    train_set_stem_source(ctx.sc);
    run_prog(step, s, ctx, false);
    if (int e = train_backward(target_nhwc, 1.0f, loss_dev, s, p2w)) return e;
    if (pred) hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)net_out.p, B, C, HW, pred);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

void Plan::run_prog(std::vector<Op>& prog, hipStream_t s, const StepCtx& ctx, bool prof) {
    static const char* op_timing = getenv("DDIF_OP_TIMING");
    if (op_timing && prof && !op_timing_done) {  // development aid: every op of ONE step between its own pair of events
        op_timing_done = true;
        hipEvent_t e0, e1;
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            if (FILE* f = fopen(op_timing, "w")) {
                fprintf(f, "op,kernel,us,gflop,mbytes\n");
                for (auto& op : prog) {
                    (void)hipEventRecord(e0, s);
                    op.run(s, ctx);
                    (void)hipEventRecord(e1, s);
                    (void)hipEventSynchronize(e1);
                    float ms = 0.f;
                    (void)hipEventElapsedTime(&ms, e0, e1);
                    fprintf(f, "\"%s\",%s,%.2f,%.4f,%.3f\n", op.label.empty() ? op.name : op.label.c_str(), op.name, ms * 1e3, op.flop / 1e9, op.bytes / 1e6);
                }
                fclose(f);
                (void)hipEventDestroy(e0);
                (void)hipEventDestroy(e1);
                return;
            }
        }
    }
    // a step is profiled completely or not at all: per-step figures divide by prof_steps
    if (prof && ev_used + (int)prog.size() > (int)ev0.size()) prof = false;
    if (prof) ++prof_steps;
    for (auto& op : prog) {
        const bool t = prof && (op.timed || prof_all) && ev_used < (int)ev0.size();
        if (t) (void)hipEventRecord(ev0[ev_used], s);
        op.run(s, ctx);
        if (t) {
            (void)hipEventRecord(ev1[ev_used], s);
            ev_flop[ev_used] = op.flop;
            ev_mflop[ev_used] = op.flop * op.mfma_w;
            ev_bytes[ev_used] = op.bytes;
            ev_cls[ev_used] = op.cls;
            ++ev_used;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entry points
int Plan::set_cond(const float* cond, hipStream_t s) {
    if (!cond) return fail(DDIF_ERR_INVALID, "ddif_plan_set_cond: cond is NULL");
    cond_nchw = const_cast<float*>(cond);
    StepCtx ctx;
    if (train_mode && wg_async) {
        // encoder half (and everything shared) on the caller's stream, then the decoder-only half -- kv convs, contexts, padded copies for the weight
        // gradients -- on the side stream: it overlaps the stem / encoder / middle of the forward pass that follows, which joins in front of its
        // first decoder block.  (Encoder ops all precede decoder ops in `pre`; the side ops depend on the resized cond images only.)
        train_join(s);  // a previous set_cond's side work may still be reading what the ops below rewrite
        for (auto& op : pre)
            if (!op.side) op.run(s, ctx);
        hipStream_t ws = train_fork(s);
        for (auto& op : pre)
            if (op.side) op.run(ws, ctx);
        (void)hipEventRecord(side_read, ws);  // ddif_net_refresh waits for this before it rewrites the weight packs these ops read
        side_pending = true;
    } else {
        run_prog(pre, s, ctx, false);
    }
    cond_set = true;
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

int Plan::forward(const float* x, const float* t_host, const float* sc, float* out, hipStream_t s) {
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_forward before ddif_plan_set_cond");
    if (!x || !t_host || !out) return fail(DDIF_ERR_INVALID, "ddif_plan_forward: NULL argument");
    const int HW = H * W, Cx = net->cfg.in_channel;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid((size_t)B * HW * Cx), dim3(256), 0, s, x, B, Cx, HW, 0, Cx, x_in.p);
    if (sc) hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid((size_t)B * HW * C), dim3(256), 0, s, sc, B, C, HW, 0, C, sc_in.p);
    if (int e = time_rows(t_host, B, s)) return e;
    StepCtx ctx;
    ctx.x = x_in.p;
    ctx.sc = sc ? sc_in.p : x_in.p;
    ctx.tb = tb;
    ctx.tb_stride = net->nslots;
    run_prog(step, s, ctx, false);
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid((size_t)B * HW * C), dim3(256), 0, s, (const float*)net_out.p, B, C, HW, out);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

// TEST-ONLY (include/ddif_testops.h ddif_plan_forward_taps): forward() launch by launch -- plain stream launches, no profiling -- with a layout-converting copy
// (NHWC arena tensor -> caller's NCHW buffer) of every requested tap right behind the launch that completes it: the arena reuses the memory later in the step.
int Plan::forward_taps(const float* x, const float* t_host, const float* sc, float* out, int n, const int* ids, float* const* dst, hipStream_t s) {
    if (train_mode) return fail(DDIF_ERR_STATE, "ddif_plan_forward_taps: inference plans only");
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_forward_taps before ddif_plan_set_cond");
    if (!x || !t_host || !out || n < 0 || (n > 0 && (!ids || !dst))) return fail(DDIF_ERR_INVALID, "ddif_plan_forward_taps: NULL argument");
    for (int k = 0; k < n; ++k) {
        if (ids[k] < 0 || ids[k] >= (int)taps.size() || !dst[k]) return fail(DDIF_ERR_INVALID, "ddif_plan_forward_taps: tap %d of %d / NULL buffer", ids[k], (int)taps.size());
        const Tap& tp = taps[ids[k]];
        if (tp.op < 0 || tp.op >= (int)(tp.cond_only ? pre.size() : step.size())) return fail(DDIF_ERR_STATE, "ddif_plan_forward_taps: tap %s has no producer", tp.name.c_str());
    }
    auto copy_out = [&](int k) {
        const Tap& tp = taps[ids[k]];
        hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid((size_t)B * tp.t.H * tp.t.W * tp.t.C), dim3(256), 0, s, (const float*)tp.t.p, B, tp.t.C, tp.t.H * tp.t.W, dst[k]);
    };
    const int HW = H * W, Cx = net->cfg.in_channel;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid((size_t)B * HW * Cx), dim3(256), 0, s, x, B, Cx, HW, 0, Cx, x_in.p);
    if (sc) hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid((size_t)B * HW * C), dim3(256), 0, s, sc, B, C, HW, 0, C, sc_in.p);
    if (int e = time_rows(t_host, B, s)) return e;
    for (int k = 0; k < n; ++k)
        if (taps[ids[k]].cond_only) copy_out(k);  // caches of the set_cond program: complete since set_cond, never aliased
    StepCtx ctx;
    ctx.x = x_in.p;
    ctx.sc = sc ? sc_in.p : x_in.p;
    ctx.tb = tb;
    ctx.tb_stride = net->nslots;
    for (int i = 0; i < (int)step.size(); ++i) {
        step[i].run(s, ctx);
        for (int k = 0; k < n; ++k)
            if (!taps[ids[k]].cond_only && taps[ids[k]].op == i) copy_out(k);
    }
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid((size_t)B * HW * C), dim3(256), 0, s, (const float*)net_out.p, B, C, HW, out);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

// The sticky range flag of the plan's raw-input f16x2 convs: read (and cleared) once per sampler / forward call by the caller, never inside a loop.
int Plan::range_status(hipStream_t s, int* overflow) {
    int v = 0;
    if (d_range && n_range_convs > 0) {
        DDIF_HIPCHK(hipMemcpyAsync(&v, d_range, sizeof(int), hipMemcpyDeviceToHost, s));
        DDIF_HIPCHK(hipStreamSynchronize(s));
        if (v) DDIF_HIPCHK(hipMemsetAsync(d_range, 0, sizeof(int), s));
    }
    if (overflow) *overflow = v ? 1 : 0;
    return 0;
}

static const char* const TILING_NO_SOLVER =
    "the plan is tiled (ddif_plan_set_tiling) and per-step fusion inside solver programs is not implemented -- turn tiling off, sample the tiles independently and blend "
    "them once at the end (\"final\" blending, ddif_tiles_blend)";
static int check_sampler_net(const Net* n) {
    if (n->cfg.in_channel != n->cfg.out_channel)
        return fail(DDIF_ERR_INVALID, "samplers need in_channel == out_channel (x_start prediction over the image channels)");
    return 0;
}

// Shared loop of the DDPM (kind 0) and DDIM (kind 1) samplers.  Everything that changes from step to step is read
// from device memory (step counter, coefficient tables, SamplerRun), so two consecutive steps (img0 -> img1 -> img0)
// are captured ONCE into a hipGraph and replayed: ~270 launches per replay instead of per-kernel host launches.
int Plan::run_sampler(int kind, int n_steps, const float* const* tabs_host, int n_tabs, const ddif_pred_tables* pred_tabs, const float* t_model, const float* xT,
                      const float* noise, uint64_t seed, uint64_t tile0, float lo, float hi, int do_clamp, float* out, hipStream_t s) {
    if (int e = check_sampler_net(net)) return e;
    if (tiling_on && kind == 0 && thr_mode == DDIF_THRESHOLD_DDPM)
        return fail(DDIF_ERR_INVALID, "ddif_plan_sample_ddpm: dynamic thresholding (ddif_plan_set_threshold mode 1) under tiling -- the per-tile s_b would differ between the covers of a pixel");
    if (side_pending) {  // a train-mode plan: the cond-only side work must not be waited for inside a captured step
        train_join(s);
        side_pending = false;
    }
    const int HW = H * W;
    const size_t n = (size_t)B * HW * C;
    if (xT) hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, xT, B, C, HW, 0, C, img[0]);
    else if (tiling_on) randn_tiled_launch(img[0], C, ttab, (unsigned long long)seed, 0u, (unsigned long long)tile0, s);  // keyed by scene pixel: every cover draws the same normal
    else hipLaunchKernelGGL(randn_nhwc_kernel, ew_grid(n), dim3(256), 0, s, img[0], B, C, HW, (unsigned long long)seed, 0u, (unsigned long long)tile0);
    if (int e = time_rows(t_model, n_steps, s)) return e;
    if (!d_step) {
        if (int e = dalloc(&d_step, 16)) return e;
        SamplerRun* r = nullptr;
        if (int e = dalloc(&r, 1)) return e;
        d_run = r;
    }
    if (tabs_cap < n_steps) {
        drop_graphs();
        if (int e = dalloc(&d_tabs, (size_t)8 * n_steps)) return e;
        tabs_cap = n_steps;
    }
    SamplerRun run{};
    run.noise = noise;
    run.seed = seed;
    run.tile0 = tile0;
    run.lo = lo;
    run.hi = hi;
    run.do_clamp = do_clamp;
    run.n_steps = n_steps;
    for (int i = 0; i < n_tabs; ++i) {
        run.tab[i] = d_tabs + (size_t)i * tabs_cap;
        DDIF_HIPCHK(hipMemcpyAsync(d_tabs + (size_t)i * tabs_cap, tabs_host[i], (size_t)n_steps * sizeof(float), hipMemcpyHostToDevice, s));
    }
    const bool pred = pred_mode != DDIF_PRED_X_START;
    if (pred) {  // the two coefficients of the prediction -> x0 conversion (sampler_dev.h pred_x0)
        if (!pred_tabs || pred_tabs->n_steps != n_steps || !pred_tabs->coef_xt || !pred_tabs->coef_out)
            return fail(DDIF_ERR_INVALID, "sampler: the plan's objective is a noise / v prediction (ddif_plan_set_objective) -- the _ex entry point with ddif_pred_tables of %d steps is needed", n_steps);
        const float* pt[2] = {pred_tabs->coef_xt, pred_tabs->coef_out};
        for (int i = 0; i < 2; ++i) {
            run.tab[6 + i] = d_tabs + (size_t)(6 + i) * tabs_cap;
            DDIF_HIPCHK(hipMemcpyAsync(d_tabs + (size_t)(6 + i) * tabs_cap, pt[i], (size_t)n_steps * sizeof(float), hipMemcpyHostToDevice, s));
        }
    }
    // dynamic thresholding (DDPM only, and only where the reference clips at all: p_sample_loop's clip_noise gates both clamps, :447; ddim_sample never clamps
    // dynamically): s_b needs the whole sample, which the final conv's epilogue cannot see -> the unfused tail with the quantile kernel in front of the update
    const bool dyn = thr_mode == DDIF_THRESHOLD_DDPM && kind == 0 && do_clamp;
    if (kind == 0 && graph_exec[0] && graph_dyn != dyn) drop_graphs();
    // tiling: the fusion needs x_{t-1} of every cover, which the final conv's epilogue of one tile cannot see -> the unfused tail as well, the fusion behind the update
    const bool fused = !dyn && !tiling_on && (pred ? final_fused_pred : final_fused);
    QuantArgs qa{};
    if (dyn) {
        qa.a = net_out.p;
        qa.lms = lms.p;
        qa.n = (long long)HW * C;
        qa.form = QUANT_DDPM;
        qa.pred = pred ? 1 : 0;
        qa.run = reinterpret_cast<const SamplerRun*>(d_run);
        quantile_rank(thr_ratio, qa.n, &qa.k_lo, &qa.k_hi, &qa.w);
        qa.max_val = thr_max;
        qa.s_out = d_thr;
    }
    DDIF_HIPCHK(hipMemcpyAsync(d_run, &run, sizeof(run), hipMemcpyHostToDevice, s));
    DDIF_HIPCHK(hipMemsetAsync(d_step, 0, 2 * sizeof(int), s));
    // the host copies above must have been consumed before `run` (stack) goes away: pageable H2D copies are staged
    // synchronously by the runtime, so returning after the enqueue is safe.

    auto one_step = [&](int parity, hipStream_t st, bool prof) {
        StepCtx ctx;
        ctx.x = ctx.sc = img[parity];  // self-conditioning == current image (diffusion_ddpm_pan.py:491,502; sr3_dwt.py:173)
        ctx.tb = tb;
        ctx.tb_stride = 0;
        ctx.step_ptr = d_step + parity;
        ctx.step_next = d_step + (parity ^ 1);
        ctx.samp_run = d_run;
        ctx.samp_kind = kind;
        ctx.samp_out = fused ? img[parity ^ 1] : nullptr;
        ctx.samp_pred = pred;
        ctx.tb_rowstride = net->nslots;
        run_prog(step, st, ctx, prof);
        StepArgs a{};
        a.x0 = net_out.p;
        a.img = img[parity];
        a.lms = lms.p;
        a.out = img[parity ^ 1];
        a.B = B;
        a.C = C;
        a.HW = HW;
        a.run = reinterpret_cast<const SamplerRun*>(d_run);
        a.pred = pred ? 1 : 0;
        if (fused) return;  // the update ran in the final conv's epilogue, which also wrote the next step's counter
        a.step = d_step + parity;
        if (dyn) {
            QuantArgs q = qa;
            q.xt = img[parity];
            q.step = d_step + parity;
            quantile_launch(q, B, st);
            a.thr = d_thr;
        }
        if (tiling_on) a.tile = ttab;
        if (kind == 0) hipLaunchKernelGGL(ddpm_step_kernel, ew_grid(n), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(ddim_step_kernel, ew_grid(n), dim3(256), 0, st, a);
        if (tiling_on) tile_fuse_launch(img[parity ^ 1], C, ttab, st);
        hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, st, (const int*)(d_step + parity), d_step + (parity ^ 1));
    };

    bool graph_ok = false;
    (void)graph_ok;
#ifndef DDIF_EMU
    static const bool graph_env = env_flag("DDIF_GRAPH", true);
    if (use_graph && graph_env && n_steps >= 4) {
        if (!graph_exec[kind]) {
            if (!cap_stream) DDIF_HIPCHK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
            hipGraph_t g = nullptr;
            hipError_t e1 = hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal);
            if (e1 == hipSuccess) {
                one_step(0, cap_stream, false);
                one_step(1, cap_stream, false);
                e1 = hipStreamEndCapture(cap_stream, &g);
            }
            hipGraphExec_t ge = nullptr;
            if (e1 == hipSuccess && g) e1 = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            if (g) (void)hipGraphDestroy(g);
            if (e1 == hipSuccess && ge) {
                graph_exec[kind] = ge;
                if (kind == 0) graph_dyn = dyn;
            } else {
                (void)hipGetLastError();
                use_graph = false;  // capture unsupported here: plain stream launches (same kernels, same results)
            }
        }
        graph_ok = graph_exec[kind] != nullptr;
    }
#endif
    int k = 0;
    while (k < n_steps) {
        const bool pair = k + 1 < n_steps;
        const bool prof = prof_every > 0 && ((k % prof_every) == 0 || (pair && ((k + 1) % prof_every) == 0));
        (void)prof;
#ifndef DDIF_EMU
        if (graph_ok && pair && !prof) {
            DDIF_HIPCHK(hipGraphLaunch((hipGraphExec_t)graph_exec[kind], s));
            k += 2;
            continue;
        }
#endif
        one_step(0, s, prof_every > 0 && (k % prof_every) == 0);
        ++k;
        if (pair) {
            one_step(1, s, prof_every > 0 && (k % prof_every) == 0);
            ++k;
        }
    }
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)img[n_steps & 1], B, C, HW, out);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

// ---- train mode: dropout / DropPath masks
int Plan::train_set_dropout(int site, const float* mask_nchw, hipStream_t s) {
    if (!train_mode) return fail(DDIF_ERR_STATE, "not a train-mode plan (ddif_plan_create_train)");
    if (site < 0 || site >= (int)drop_sites.size() || !mask_nchw) return fail(DDIF_ERR_INVALID, "ddif_plan_train_set_dropout: bad site %d of %d", site, (int)drop_sites.size());
    const DropSite& d = drop_sites[site];
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid((size_t)B * d.H * d.W * d.C), dim3(256), 0, s, mask_nchw, B, d.C, d.H * d.W, 0, d.C, d.mask);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}
int Plan::train_set_droppath(const float* scales_host, hipStream_t s) {
    if (!train_mode) return fail(DDIF_ERR_STATE, "not a train-mode plan (ddif_plan_create_train)");
    if (!scales_host) return fail(DDIF_ERR_INVALID, "ddif_plan_train_set_droppath: NULL");
    for (size_t k = 0; k < path_sites.size(); ++k)
        DDIF_HIPCHK(hipMemcpyAsync(path_sites[k], scales_host + k * B, (size_t)B * sizeof(float), hipMemcpyHostToDevice, s));
    return 0;
}
int Plan::train_get_dropout(int site, float* mask_nchw, hipStream_t s) {
    if (!train_mode) return fail(DDIF_ERR_STATE, "not a train-mode plan (ddif_plan_create_train)");
    if (site < 0 || site >= (int)drop_sites.size() || !mask_nchw) return fail(DDIF_ERR_INVALID, "ddif_plan_train_get_dropout: bad site %d of %d", site, (int)drop_sites.size());
    const DropSite& d = drop_sites[site];
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid((size_t)B * d.H * d.W * d.C), dim3(256), 0, s, (const float*)d.mask, B, d.C, d.H * d.W, mask_nchw);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}
int Plan::train_get_droppath(float* scales_dev, hipStream_t s) {
    if (!train_mode) return fail(DDIF_ERR_STATE, "not a train-mode plan (ddif_plan_create_train)");
    if (!scales_dev) return fail(DDIF_ERR_INVALID, "ddif_plan_train_get_droppath: NULL");
    for (size_t k = 0; k < path_sites.size(); ++k)
        DDIF_HIPCHK(hipMemcpyAsync(scales_dev + k * B, path_sites[k], (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
int Plan::train_random_masks(uint64_t seed, uint64_t tile0, float p_drop, float p_path, hipStream_t s) {
    if (!train_mode) return fail(DDIF_ERR_STATE, "not a train-mode plan (ddif_plan_create_train)");
    if (!(p_drop >= 0.f && p_drop < 1.f && p_path >= 0.f && p_path < 1.f)) return fail(DDIF_ERR_INVALID, "drop probabilities must be in [0, 1)");
    if (!mask_recs) {  // the table of sites (fixed for the life of the plan): dropout sites first, DropPath sites after them, numbered in that order
        std::vector<MaskRec> tab;
        unsigned long long blk = 0;
        auto push = [&](float* m, int C_, int HW_, int path) {
            MaskRec r{};
            r.mask = m;
            r.C = C_;
            r.HW = HW_;
            r.site = (unsigned)tab.size();
            r.path = path;
            r.blk0 = blk;
            const size_t units = (HW_ & 3) == 0 ? (size_t)B * (HW_ >> 2) * C_ : (size_t)B * HW_ * C_;
            blk += (units + MASK_QPB - 1) / MASK_QPB;
            tab.push_back(r);
        };
        for (const DropSite& d : drop_sites) push(d.mask, d.C, d.H * d.W, 0);
        for (float* p : path_sites) push(p, 1, 1, 1);
        if (tab.empty()) return 0;
        float* raw = nullptr;
        if (int e = dalloc(&raw, (tab.size() * sizeof(MaskRec) + sizeof(float) - 1) / sizeof(float))) return e;
        DDIF_HIPCHK(hipMemcpy(raw, tab.data(), tab.size() * sizeof(MaskRec), hipMemcpyHostToDevice));
        mask_recs = raw;
        n_mask_recs = (int)tab.size();
        mask_blocks = blk;
    }
    hipLaunchKernelGGL(train_masks_kernel, dim3((unsigned)mask_blocks), dim3(256), 0, s, reinterpret_cast<const MaskRec*>(mask_recs), n_mask_recs, B,
                       (unsigned long long)seed, (unsigned long long)tile0, 1.f - p_drop, 1.f - p_path);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

int Plan::sample_ddpm(const ddif_ddpm_tables* t, const ddif_pred_tables* pt, const float* xT, const float* noise, uint64_t seed, uint64_t tile0,
                      float lo, float hi, int do_clamp, float* out, hipStream_t s) {
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_sample_ddpm before ddif_plan_set_cond");
    if (!t || t->n_steps < 1 || !t->t_model || !t->coef_x0 || !t->coef_xt || !t->coef_z || !out)
        return fail(DDIF_ERR_INVALID, "ddif_plan_sample_ddpm: bad tables");
    const float* tabs[3] = {t->coef_x0, t->coef_xt, t->coef_z};
    return run_sampler(0, t->n_steps, tabs, 3, pt, t->t_model, xT, noise, seed, tile0, lo, hi, do_clamp, out, s);
}

int Plan::sample_ddim(const ddif_ddim_tables* t, const ddif_pred_tables* pt, const float* xT, const float* noise, uint64_t seed, uint64_t tile0,
                      float lo, float hi, int do_clamp, float* out, hipStream_t s) {
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_sample_ddim before ddif_plan_set_cond");
    if (!t || t->n_steps < 1 || !t->t_model || !t->sqrt_recip || !t->sqrt_recipm1 || !t->sqrt_ap || !t->dir_coef || !t->sigma || !out)
        return fail(DDIF_ERR_INVALID, "ddif_plan_sample_ddim: bad tables");
    const float* tabs[5] = {t->sqrt_recip, t->sqrt_recipm1, t->sqrt_ap, t->dir_coef, t->sigma};
    return run_sampler(1, t->n_steps, tabs, 5, pt, t->t_model, xT, noise, seed, tile0, lo, hi, do_clamp, out, s);
}

int Plan::sample_dpmpp(const ddif_dpm_tables* t, const float* xT, float lo, float hi, int do_clamp, float* out, hipStream_t s) {
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_sample_dpmpp before ddif_plan_set_cond");
    if (!t || t->n_evals < 1 || t->order < 1 || t->order > 3 || !t->t_model || !t->alpha || !t->sigma || !t->ord || !t->cx || !t->a_phi1 || !xT || !out)
        return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpmpp: bad tables");
    if (int e = check_sampler_net(net)) return e;
    if (tiling_on) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpmpp: %s", TILING_NO_SOLVER);
    const bool dyn = thr_mode == DDIF_THRESHOLD_SOLVER;
    if (dyn && do_clamp)
        return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpmpp: the plan thresholds dynamically (ddif_plan_set_threshold mode 2) -- the image-space clamp is the other corrector, not an addition");
    if (side_pending) {
        train_join(s);
        side_pending = false;
    }
    const int HW = H * W;
    const size_t n = (size_t)B * HW * C;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, xT, B, C, HW, 0, C, img[0]);
    if (int e = time_rows(t->t_model, t->n_evals, s)) return e;
    QuantArgs qa{};
    if (dyn) {
        qa.a = net_out.p;
        qa.n = (long long)HW * C;
        qa.form = QUANT_DPM;
        qa.pred = pred_mode;
        quantile_rank(thr_ratio, qa.n, &qa.k_lo, &qa.k_hi, &qa.w);
        qa.max_val = thr_max;
        qa.s_out = d_thr;
    }
    int cur = 0;
    float* hist[3] = {nullptr, nullptr, nullptr};  // newest first
    int nhist = 0, slot = 0;
    for (int k = 0; k < t->n_evals; ++k) {
        StepCtx ctx;
        ctx.x = ctx.sc = img[cur];  // model_wrapper never passes self_cond (dpm_solver.py:295) -> x
        ctx.tb = tb + (size_t)k * net->nslots;
        const bool prof = prof_every > 0 && (k % prof_every) == 0;
        run_prog(step, s, ctx, prof);
        float* mnew = mbuf[slot];
        slot = (slot + 1) % 3;
        if (dyn) {  // s_b of this evaluation's x0 (solver/dpm_solver.py:424-433), on the device: nothing comes back to the host
            QuantArgs q = qa;
            q.xt = img[cur];
            q.alpha = t->alpha[k];
            q.sigma = t->sigma[k];
            quantile_launch(q, B, s);
        }
        hipLaunchKernelGGL(dpm_x0_kernel, ew_grid(n), dim3(256), 0, s, (const float*)net_out.p, (const float*)img[cur], (const float*)lms.p,
                           t->alpha[k], t->sigma[k], lo, hi, do_clamp, pred_mode, n, mnew, (const float*)(dyn ? d_thr : nullptr), (size_t)HW * C);
        hist[2] = hist[1];
        hist[1] = hist[0];
        hist[0] = mnew;
        if (nhist < 3) ++nhist;
        const int o = t->ord[k];
        if (o < 1 || o > nhist) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpmpp: update %d has order %d with %d model values", k, o, nhist);
        DpmUpdArgs u{};
        u.x = img[cur];
        u.m0 = hist[0];
        u.m1 = o >= 2 ? hist[1] : nullptr;
        u.m2 = o >= 3 ? hist[2] : nullptr;
        u.out = img[cur ^ 1];
        u.n = n;
        u.order = o;
        u.cx = t->cx[k];
        u.a1 = t->a_phi1[k];
        u.inv_r0 = (o >= 2 && t->inv_r0) ? t->inv_r0[k] : 0.f;
        u.inv_r1 = (o >= 3 && t->inv_r1) ? t->inv_r1[k] : 0.f;
        u.r0_frac = (o >= 3 && t->r0_frac) ? t->r0_frac[k] : 0.f;
        u.inv_r01 = (o >= 3 && t->inv_r01) ? t->inv_r01[k] : 0.f;
        u.a2 = (o >= 3 && t->a_phi2) ? t->a_phi2[k] : 0.f;
        u.a3 = (o >= 3 && t->a_phi3) ? t->a_phi3[k] : 0.f;
        hipLaunchKernelGGL(dpm_update_kernel, ew_grid(n), dim3(256), 0, s, u);
        cur ^= 1;
    }
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)img[cur], B, C, HW, out);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

// A host-built solver program (include/ddif.h ddif_dpm_program; reference solver/dpm_solver.py:1055-1253).  Validated as a whole before the first launch.
int Plan::sample_dpm(const ddif_dpm_program* prog, const float* xT, float lo, float hi, int do_clamp, float* out, float* inter_out, hipStream_t s) {
    return run_dpm_program(prog, false, 1.f, xT, lo, hi, do_clamp, out, inter_out, s);
}

// Classifier-free guidance (model_wrapper, solver/dpm_solver.py:330-338): the plan's batch is [unconditional (Bg); conditional (Bg)], the program and its
// launches are those of sample_dpm at that batch, and dpm_eval_update_kernel combines the two halves of every network output before anything else sees it.
int Plan::sample_dpm_guided(const ddif_dpm_program* prog, float guidance_scale, const float* xT, float lo, float hi, int do_clamp, float* out, float* inter_out,
                            hipStream_t s) {
    if (!prog || !prog->ops || !xT || !out) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm_guided: NULL program, op table, x_T or out");
    if (!std::isfinite(guidance_scale)) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm_guided: guidance_scale is not finite");
    if (B % 2) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm_guided: the plan's batch %d is odd -- it holds [unconditional; conditional], two halves of equal size", B);
    return run_dpm_program(prog, true, guidance_scale, xT, lo, hi, do_clamp, out, inter_out, s);
}

// guided: xT, out and every inter_out slice hold B / 2 images; state registers hold the same bits in both halves, model registers use their first half only.
int Plan::run_dpm_program(const ddif_dpm_program* prog, bool guided, float gscale, const float* xT, float lo, float hi, int do_clamp, float* out, float* inter_out,
                          hipStream_t s) {
    if (!cond_set) return fail(DDIF_ERR_STATE, "%s before ddif_plan_set_cond", guided ? "ddif_plan_sample_dpm_guided" : "ddif_plan_sample_dpm");
    if (!prog || !prog->ops || prog->n_ops < 1 || !xT || !out) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: NULL program, op table, x_T or out");
    if (prog->algorithm != DDIF_DPM_ALGO_DPMSOLVERPP && prog->algorithm != DDIF_DPM_ALGO_DPMSOLVER)
        return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: algorithm %d (0 dpmsolver++, 1 dpmsolver)", prog->algorithm);
    if (int e = check_sampler_net(net)) return e;
    if (tiling_on) return fail(DDIF_ERR_INVALID, "%s: %s", guided ? "ddif_plan_sample_dpm_guided" : "ddif_plan_sample_dpm", TILING_NO_SOLVER);
    const bool dyn = thr_mode == DDIF_THRESHOLD_SOLVER;
    if (dyn && do_clamp)
        return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: the plan thresholds dynamically (ddif_plan_set_threshold mode 2) -- the image-space clamp is the other corrector, not an addition");
    const int NR = DDIF_DPM_NUM_REGS;
    auto reg_ok = [NR](int r) { return r >= 0 && r < NR; };
    bool st_set[DDIF_DPM_NUM_REGS] = {true, false, false}, m_set[DDIF_DPM_NUM_REGS] = {false, false, false};
    bool need_reg2 = false;
    std::vector<float> t_model;
    for (int k = 0; k < prog->n_ops; ++k) {
        const ddif_dpm_op& op = prog->ops[k];
        if (op.kind == DDIF_DPM_EVAL || op.kind == DDIF_DPM_FINAL_DENOISE) {
            if (!reg_ok(op.src) || !reg_ok(op.dst)) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d names register %d -> %d (0..%d)", k, op.src, op.dst, NR - 1);
            if (!st_set[op.src]) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d evaluates state register %d before it is written", k, op.src);
            if (op.kind == DDIF_DPM_EVAL) m_set[op.dst] = true;
            else st_set[op.dst] = true;
            need_reg2 |= op.src == 2 || (op.kind == DDIF_DPM_FINAL_DENOISE && op.dst == 2);
            t_model.push_back(op.t_model);
        } else if (op.kind == DDIF_DPM_UPDATE) {
            if (!reg_ok(op.src) || !reg_ok(op.dst)) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d names register %d -> %d (0..%d)", k, op.src, op.dst, NR - 1);
            if (!st_set[op.src]) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d updates state register %d before it is written", k, op.src);
            int nm = 0;
            if (op.form == DDIF_DPM_FORM_MULTI) {
                if (op.order < 1 || op.order > 3) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d has order %d (1..3)", k, op.order);
                nm = op.order;
            } else if (op.form == DDIF_DPM_FORM_LIN1) nm = 1;
            else if (op.form == DDIF_DPM_FORM_LIN2 || op.form == DDIF_DPM_FORM_TAY3) nm = 3;
            else return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d has update form %d", k, op.form);
            for (int j = 0; j < nm; ++j) {
                if (!reg_ok(op.m[j])) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d names model register %d (0..%d)", k, op.m[j], NR - 1);
                if (!m_set[op.m[j]]) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d reads model register %d before it is written", k, op.m[j]);
            }
            st_set[op.dst] = true;
            need_reg2 |= op.src == 2 || op.dst == 2;
        } else if (op.kind == DDIF_DPM_EMIT) {
            if (!reg_ok(op.src)) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d names register %d (0..%d)", k, op.src, NR - 1);
            if (!st_set[op.src]) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d emits state register %d before it is written", k, op.src);
            if (!inter_out) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d emits an intermediate but inter_out is NULL", k);
            need_reg2 |= op.src == 2;
        } else {
            return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: op %d has kind %d", k, op.kind);
        }
    }
    if (t_model.empty()) return fail(DDIF_ERR_INVALID, "ddif_plan_sample_dpm: the program evaluates the network nowhere");
    if (side_pending) {
        train_join(s);
        side_pending = false;
    }
    const int HW = H * W;
    const int Bo = guided ? B / 2 : B;  // images in x_T, out and an inter_out slice
    const size_t nfull = (size_t)B * HW * C;
    const size_t n = (size_t)Bo * HW * C;  // work items of an elementwise launch
    const size_t half = guided ? n : 0;
    if (need_reg2 && !xreg2)
        if (int e = dalloc(&xreg2, nfull)) return e;
    float* const st[DDIF_DPM_NUM_REGS] = {img[0], img[1], xreg2};
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, xT, Bo, C, HW, 0, C, img[0]);
    if (guided) hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, xT, Bo, C, HW, 0, C, img[0] + half);  // x_in = cat([x, x]) (:334)
    if (int e = time_rows(t_model.data(), (int)t_model.size(), s)) return e;
    QuantArgs qa{};
    if (dyn) {
        qa.a = net_out.p;
        if (guided) {  // one s_b per guided sample, from the guided noise prediction
            qa.a2 = net_out.p + half;
            qa.gscale = gscale;
        }
        qa.n = (long long)HW * C;
        qa.form = QUANT_DPM;
        qa.pred = pred_mode;
        quantile_rank(thr_ratio, qa.n, &qa.k_lo, &qa.k_hi, &qa.w);
        qa.max_val = thr_max;
        qa.s_out = d_thr;
    }
    auto set_update = [&](DpmEvalArgs& a, const ddif_dpm_op& u) {
        a.form = u.form == DDIF_DPM_FORM_MULTI ? DPM_FORM_MULTI : u.form == DDIF_DPM_FORM_TAY3 ? DPM_FORM_TAY3 : DPM_FORM_LIN2;
        a.order = u.order;
        a.x = st[u.src];
        a.out = st[u.dst];
        const int nm = u.form == DDIF_DPM_FORM_MULTI ? u.order : u.form == DDIF_DPM_FORM_LIN1 ? 1 : 3;
        a.m0 = mbuf[u.m[0]];
        a.m1 = nm >= 2 ? mbuf[u.m[1]] : nullptr;
        a.m2 = nm >= 3 ? mbuf[u.m[2]] : nullptr;
        for (int j = 0; j < 9; ++j) a.c[j] = u.c[j];
    };
    int row = 0, emitted = 0;
    for (int k = 0; k < prog->n_ops; ++k) {
        const ddif_dpm_op& op = prog->ops[k];
        if (op.kind == DDIF_DPM_EMIT) {
            hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)st[op.src], Bo, C, HW, inter_out + (size_t)emitted * n);
            ++emitted;
            continue;
        }
        DpmEvalArgs a{};
        a.n = n;
        a.per = (size_t)HW * C;
        a.half = half;
        a.gscale = gscale;
        if (op.kind == DDIF_DPM_UPDATE) {  // an update on its own (the program did not put it behind an evaluation)
            set_update(a, op);
            hipLaunchKernelGGL(dpm_eval_update_kernel, ew_grid(n), dim3(256), 0, s, a);
            continue;
        }
        const bool fin = op.kind == DDIF_DPM_FINAL_DENOISE;
        const bool data = fin || prog->algorithm == DDIF_DPM_ALGO_DPMSOLVERPP;  // the final denoise is the data prediction with its corrector under either algorithm (:549-553)
        StepCtx ctx;
        ctx.x = ctx.sc = st[op.src];  // model_wrapper never passes self_cond (dpm_solver.py:295) -> x
        ctx.tb = tb + (size_t)row * net->nslots;
        const bool prof = prof_every > 0 && (row % prof_every) == 0;
        ++row;
        run_prog(step, s, ctx, prof);
        if (dyn && data) {  // s_b of this evaluation's x0 (solver/dpm_solver.py:424-433), on the device
            QuantArgs q = qa;
            q.xt = st[op.src];
            q.alpha = op.alpha;
            q.sigma = op.sigma;
            quantile_launch(q, Bo, s);
        }
        a.net = net_out.p;
        a.xe = st[op.src];
        a.lms = lms.p;
        a.thr = (dyn && data) ? d_thr : nullptr;
        a.alpha = op.alpha;
        a.sigma = op.sigma;
        a.lo = lo;
        a.hi = hi;
        a.do_clamp = data ? do_clamp : 0;
        a.model_type = pred_mode;
        a.eps_only = data ? 0 : 1;
        a.form = DPM_FORM_NONE;
        if (fin) {
            a.out = st[op.dst];
        } else {
            a.m_out = mbuf[op.dst];
            if (k + 1 < prog->n_ops && prog->ops[k + 1].kind == DDIF_DPM_UPDATE) set_update(a, prog->ops[++k]);  // the update behind this evaluation rides in its launch
        }
        hipLaunchKernelGGL(dpm_eval_update_kernel, ew_grid(n), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)img[0], Bo, C, HW, out);
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

int Plan::q_sample_forward(const float* x0, const float* noise, const float* a_h, const float* s_h, const float* t_h,
                           const float* sc, float* pred, hipStream_t s, const ddif_objective_rows* rows, float* recon_out) {
    if (!cond_set) return fail(DDIF_ERR_STATE, "ddif_plan_q_sample_forward before ddif_plan_set_cond");
    if (!x0 || !noise || !a_h || !s_h || !t_h || (!pred && !recon_out)) return fail(DDIF_ERR_INVALID, "ddif_plan_q_sample_forward: NULL argument");
    if (int e = check_sampler_net(net)) return e;
    if (recon_out && pred_mode != DDIF_PRED_X_START)
        if (int e = objective_rows(rows, false, s)) return e;
    const int HW = H * W;
    const size_t n = (size_t)B * HW * C;
    DDIF_HIPCHK(hipMemcpyAsync(small, a_h, (size_t)B * sizeof(float), hipMemcpyDefault, s));  // host or device source
    DDIF_HIPCHK(hipMemcpyAsync(small + B, s_h, (size_t)B * sizeof(float), hipMemcpyDefault, s));
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, x0, B, C, HW, 0, C, img[0]);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, noise, B, C, HW, 0, C, img[1]);
    hipLaunchKernelGGL(q_sample_kernel, ew_grid(n), dim3(256), 0, s, (const float*)img[0], (const float*)img[1], (const float*)small, (const float*)(small + B), B, (size_t)HW * C, x_in.p);
    if (sc) hipLaunchKernelGGL(nchw_to_nhwc_kernel, ew_grid(n), dim3(256), 0, s, sc, B, C, HW, 0, C, sc_in.p);
    if (int e = time_rows(t_h, B, s)) return e;
    StepCtx ctx;
    ctx.x = x_in.p;
    ctx.sc = sc ? sc_in.p : x_in.p;
    ctx.tb = tb;
    ctx.tb_stride = net->nslots;
    run_prog(step, s, ctx, false);
    if (pred) hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)net_out.p, B, C, HW, pred);
    if (recon_out) {  // the x0 the self-conditioning pass feeds back (:708-713)
        if (pred_mode == DDIF_PRED_X_START) hipLaunchKernelGGL(nhwc_to_nchw_kernel, ew_grid(n), dim3(256), 0, s, (const float*)net_out.p, B, C, HW, recon_out);
        else if (int e = recon(net_out.p, recon_out, true, s)) return e;
    }
    DDIF_HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace ddif

// TEST-ONLY (include/ddif_testops.h): one launch of dpm_eval_update_kernel on plain arrays; half != 0 is the guided form (n work items, two halves of n floats)
static int dpm_eval_update_launch(const char* who, const float* net, const float* xe, const float* lms, const float* thr, int64_t n, int64_t per, int64_t half, float gscale,
                                  float alpha, float sigma, float lo, float hi, int do_clamp, int model_type, int algorithm, int form, int order, const float* x,
                                  const float* m0, const float* m1, const float* m2, const float* c_host, float* m_out, float* out, void* stream) {
    using namespace ddif;
    if (n < 1 || per < 1 || (net && !xe) || (net && do_clamp && !lms) || model_type < 0 || model_type > 2 || (!net && !form))
        return fail(DDIF_ERR_INVALID, "%s: bad argument", who);
    if (form && (!x || !out || !c_host || (form != DDIF_DPM_FORM_MULTI && form != DDIF_DPM_FORM_LIN1 && form != DDIF_DPM_FORM_LIN2 && form != DDIF_DPM_FORM_TAY3) ||
                 (form == DDIF_DPM_FORM_MULTI && (order < 1 || order > 3))))
        return fail(DDIF_ERR_INVALID, "%s: bad update", who);
    const int nm = !form ? 0 : form == DDIF_DPM_FORM_MULTI ? order : form == DDIF_DPM_FORM_LIN1 ? 1 : 3;
    const float* m[3] = {m0, m1, m2};
    for (int j = 0; j < nm; ++j) {
        if (!m[j]) m[j] = (net && m_out) ? m_out : nullptr;  // NULL names the value of this launch
        if (!m[j]) return fail(DDIF_ERR_INVALID, "%s: model value %d is missing", who, j);
    }
    DpmEvalArgs a{};
    a.net = net;
    a.xe = xe;
    a.lms = lms;
    a.thr = thr;
    a.m_out = m_out;
    a.alpha = alpha;
    a.sigma = sigma;
    a.lo = lo;
    a.hi = hi;
    a.do_clamp = do_clamp;
    a.model_type = model_type;
    a.eps_only = algorithm == DDIF_DPM_ALGO_DPMSOLVER;
    a.n = (size_t)n;
    a.per = (size_t)per;
    a.half = (size_t)half;
    a.gscale = gscale;
    a.form = !form ? DPM_FORM_NONE : form == DDIF_DPM_FORM_MULTI ? DPM_FORM_MULTI : form == DDIF_DPM_FORM_TAY3 ? DPM_FORM_TAY3 : DPM_FORM_LIN2;
    a.order = order;
    a.x = x;
    a.m0 = nm >= 1 ? m[0] : nullptr;
    a.m1 = nm >= 2 ? m[1] : nullptr;
    a.m2 = nm >= 3 ? m[2] : nullptr;
    a.out = out;
    if (form) for (int j = 0; j < 9; ++j) a.c[j] = c_host[j];
    hipLaunchKernelGGL(dpm_eval_update_kernel, ew_grid((size_t)n), dim3(256), 0, (hipStream_t)stream, a);
    DDIF_HIPCHK(hipGetLastError());
    return DDIF_OK;
}
extern "C" int ddif_dpm_eval_update(const float* net, const float* xe, const float* lms, const float* thr, int64_t n, int64_t per, float alpha, float sigma, float lo, float hi,
                                    int do_clamp, int model_type, int algorithm, int form, int order, const float* x, const float* m0, const float* m1, const float* m2,
                                    const float* c_host, float* m_out, float* out, void* stream) {
    return dpm_eval_update_launch("ddif_dpm_eval_update", net, xe, lms, thr, n, per, 0, 1.f, alpha, sigma, lo, hi, do_clamp, model_type, algorithm, form, order, x, m0, m1, m2,
                                  c_host, m_out, out, stream);
}
extern "C" int ddif_dpm_eval_update_guided(const float* net, const float* xe, const float* lms, const float* thr, int64_t n_half, int64_t per, float guidance_scale, float alpha,
                                           float sigma, float lo, float hi, int do_clamp, int model_type, int algorithm, int form, int order, const float* x, const float* m0,
                                           const float* m1, const float* m2, const float* c_host, float* m_out, float* out, void* stream) {
    if (!net || !std::isfinite(guidance_scale)) return ddif::fail(DDIF_ERR_INVALID, "ddif_dpm_eval_update_guided: NULL network output or a guidance_scale that is not finite");
    return dpm_eval_update_launch("ddif_dpm_eval_update_guided", net, xe, lms, thr, n_half, per, n_half, guidance_scale, alpha, sigma, lo, hi, do_clamp, model_type, algorithm,
                                  form, order, x, m0, m1, m2, c_host, m_out, out, stream);
}
