// extern "C" entry points for the convolution family: argument validation, geometry, and the
// dispatch between the direct (vector FMA) kernels and the f32-MFMA implicit-GEMM kernels.
#include "ms_common.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include "conv_mfma.h"
#include "gconv_mfma.h"
#include "conv_thin.h"

// Profile session of the calling thread (ms_profile_kernels / ms_profile_take): nothing is recorded outside one.
static thread_local int g_prof_on = 0, g_prof_launches = 0, g_prof_products = 0;
static thread_local double g_prof_us = 0.0;
static thread_local char g_prof_kernel[MS_PROFILE_NAME_MAX] = "";

void ms_note_kernel(int products, const char* fmt, ...) {
    if (!g_prof_on) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_prof_kernel, sizeof(g_prof_kernel), fmt, ap);
    va_end(ap);
    g_prof_products = products;
}

bool ms_name_or_note(char* name, int products, const char* fmt, ...) {
    if (!name && !g_prof_on) return false;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name ? name : g_prof_kernel, MS_PROFILE_NAME_MAX, fmt, ap);
    va_end(ap);
    if (!name) g_prof_products = products;
    return name != nullptr;
}

bool ms_prof_on() { return g_prof_on != 0; }

void ms_prof_add(hipEvent_t e0, hipEvent_t e1) {
    float ms = 0.f;
    if (e0 && e1 && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
        g_prof_us += 1e3 * (double)ms;
        ++g_prof_launches;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
}

namespace {

bool make_conv(const ms_conv1d_desc* d, ConvP* p) {
    if (!d) return false;
    if (d->B <= 0 || d->Cin <= 0 || d->Lin <= 0 || d->Cout <= 0 || d->K <= 0 || d->stride <= 0 ||
        d->pad < 0 || d->dil <= 0 || d->groups <= 0)
        return false;
    if (d->Cin % d->groups || d->Cout % d->groups) return false;
    if (d->pad_mode != MS_PAD_ZERO && d->pad_mode != MS_PAD_REFLECT) return false;
    if (d->pad_mode == MS_PAD_REFLECT && d->pad >= d->Lin) return false;  // nn.ReflectionPad1d rule
    if (d->act < MS_ACT_NONE || d->act > MS_ACT_TANH) return false;
    const int eff = d->Lin + 2 * d->pad - d->dil * (d->K - 1) - 1;
    if (eff < 0) return false;
    p->B = d->B; p->Cin = d->Cin; p->Lin = d->Lin; p->Cout = d->Cout; p->K = d->K;
    p->stride = d->stride; p->pad = d->pad; p->dil = d->dil; p->groups = d->groups;
    p->Cg = d->Cin / d->groups; p->Og = d->Cout / d->groups;
    p->Lout = eff / d->stride + 1;
    p->pad_mode = d->pad_mode; p->act = d->act; p->slope = d->slope;
    if (d->in_act != MS_ACT_NONE && d->in_act != MS_ACT_LRELU) return false;
    p->in_act = d->in_act;
    return true;
}

// conv whose backward-data IS the transposed conv: channels swap roles (w layout (Cin_T, Cout_T, K)
// equals the (Cout_conv, Cin_conv, K) layout of that conv).
bool make_convt(const ms_convt1d_desc* d, ConvP* p) {
    if (!d) return false;
    if (d->B <= 0 || d->Cin <= 0 || d->Lin <= 0 || d->Cout <= 0 || d->K <= 0 || d->stride <= 0 ||
        d->pad < 0)
        return false;
    if (d->act < MS_ACT_NONE || d->act > MS_ACT_TANH) return false;
    const int Lout = (d->Lin - 1) * d->stride - 2 * d->pad + d->K;
    if (Lout <= 0) return false;
    p->B = d->B; p->Cin = d->Cout; p->Lin = Lout; p->Cout = d->Cin; p->K = d->K;
    p->stride = d->stride; p->pad = d->pad; p->dil = 1; p->groups = 1;
    p->Cg = d->Cout; p->Og = d->Cin;
    p->Lout = d->Lin;
    p->pad_mode = MS_PAD_ZERO; p->act = d->act; p->slope = d->slope;
    if (d->in_act != MS_ACT_NONE && d->in_act != MS_ACT_LRELU) return false;
    p->in_act = d->in_act;   // activation in front of the TRANSPOSED conv (on its input x)
    // consistency: the conv's own output length for Lin=Lout_T must give back Lin_T
    const int chk = (Lout + 2 * d->pad - (d->K - 1) - 1) / d->stride + 1;
    return chk == d->Lin;
}

}  // namespace

extern "C" {

int ms_version(void) { return MSYNTH_VERSION; }

void ms_profile_kernels(int on) {
    g_prof_on = on ? 1 : 0;
    g_prof_us = 0.0;
    g_prof_launches = 0;
    g_prof_products = 0;
    g_prof_kernel[0] = 0;
}

int ms_profile_take(ms_profile_record* out) {
    if (!out) return MS_ERR_INVALID_ARG;
    out->kernels = g_prof_launches;
    out->products = g_prof_products;
    out->device_us = g_prof_us;
    memcpy(out->kernel, g_prof_kernel, sizeof(out->kernel));
    g_prof_us = 0.0;
    g_prof_launches = 0;
    g_prof_products = 0;
    g_prof_kernel[0] = 0;
    return MS_OK;
}

// Debug aid (tests/conftest.py): native frames on a fatal signal.  A hipGraphLaunch / kernel-launch fault inside the runtime
// leaves Python's faulthandler with Python frames only (profiles/r03_forked_replay_segfault.txt); this handler writes the
// native backtrace of the faulting thread to stderr (async-signal-safe calls only), then re-raises with the default action.
static struct sigaction g_prev_action[32];

static void ms_crash_handler(int sig) {
    static const char head[] = "\n[msynth] fatal signal: native backtrace of the faulting thread\n";
    (void)!write(2, head, sizeof(head) - 1);
    void* frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, 2);
    // hand on to whoever was installed before (Python's faulthandler prints the interpreter frames and re-raises)
    if (sig > 0 && sig < 32) sigaction(sig, &g_prev_action[sig], nullptr);
    else signal(sig, SIG_DFL);
    raise(sig);
}

int ms_debug_install_crash_handler(void) {
    void* warm[4];
    (void)backtrace(warm, 4);              // (loads libgcc's unwinder now, not inside the handler)
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_handler = ms_crash_handler;
    sa.sa_flags = SA_NODEFER | SA_RESETHAND;
    sigemptyset(&sa.sa_mask);
    int rc = 0;
    for (int sig : {SIGSEGV, SIGBUS, SIGABRT, SIGFPE, SIGILL}) rc |= sigaction(sig, &sa, &g_prev_action[sig]);
    return rc == 0 ? MS_OK : MS_ERR_INVALID_ARG;
}

const char* ms_status_string(int status) {
    switch (status) {
        case MS_OK: return "ok";
        case MS_ERR_INVALID_ARG: return "invalid argument (null pointer, bad size or inconsistent shape)";
        case MS_ERR_UNSUPPORTED: return "configuration not supported by the MI355X kernels";
        case MS_ERR_WORKSPACE: return "workspace missing or too small";
        case MS_ERR_LAUNCH: return "HIP kernel launch failed";
        case MS_ERR_COMM: return "RCCL unavailable or an RCCL call failed (ms_comm_last_error)";
        default: return "unknown status";
    }
}

// ---- rows whose length is not a multiple of 4 on the 16-byte kernels
// The D 1024 -> 1024 k5 conv at the pooled scales runs on rows of 17 / 9 samples: no row is 16-byte aligned, so the
// split-bf16 row kernel takes its dword loader (4x the load instructions, four-wave form only): 58-74 TFLOP/s against
// 160-170 for the same layer at L = 32.  For such layers the operands are copied into rows padded with zeros to
// L' = 4 ceil(L / 4) (a few MB: microseconds), the conv runs on the padded problem through the aligned paired kernel,
// and the valid columns are copied back.  Zero columns behind a row are what the conv's zero padding reads anyway, so
// the valid outputs are unchanged; the padded outputs are discarded.  Measured (tools/scratch/microbench_pad4.py, B = 64):
// L = 17 forward 197 -> 150 us, backward 232 -> 164 us; L = 33: 267 -> 212 / 379 -> 241 us.  With fewer than ~1000
// columns (B = 32 at L = 17, any batch at L = 9) the extra columns cost more than the loader saves: not padded.
namespace {

__global__ __launch_bounds__(256) void k_pad_rows(const float* __restrict__ src, float* __restrict__ dst,
                                                 size_t n_dst, int L, int Lp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_dst) return;
    const size_t row = i / (unsigned)Lp;
    const int t = (int)(i - row * (unsigned)Lp);
    dst[i] = t < L ? src[row * (unsigned)L + t] : 0.f;
}

__global__ __launch_bounds__(256) void k_unpad_rows(const float* __restrict__ src, const float* __restrict__ add,
                                                   float* __restrict__ dst, size_t n_dst, int L, int Lp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_dst) return;
    const size_t row = i / (unsigned)L;
    const int t = (int)(i - row * (unsigned)L);
    const float v = src[row * (unsigned)Lp + t];
    dst[i] = add ? v + add[i] : v;
}

bool pad4_applicable(const ConvP& p) {
    return p.groups == 1 && p.stride == 1 && p.Lout == p.Lin && (p.Lin & 3) != 0 && p.Lin >= 5 && p.Lin <= 256 &&
           (long long)p.B * p.Lin >= 1000 &&
           p.K == 5 && p.Cin >= 256 && p.Cout >= 256 && p.Cin % 16 == 0 && p.Cout % 16 == 0 &&
           p.pad_mode == MS_PAD_ZERO && !p.in_act;
}

ConvP pad4_conv(const ConvP& p) {
    ConvP q = p;
    q.Lin = q.Lout = (p.Lin + 3) & ~3;
    return q;
}

size_t pad4_bytes(const ConvP& q, int channels) { return (size_t)q.B * channels * q.Lin * sizeof(float); }

int pad_rows(const float* src, float* dst, size_t rows, int L, int Lp, hipStream_t s) {
    const size_t n = rows * (size_t)Lp;
    hipLaunchKernelGGL(k_pad_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n, L, Lp);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

int unpad_rows(const float* src, const float* add, float* dst, size_t rows, int L, int Lp, hipStream_t s) {
    const size_t n = rows * (size_t)L;
    hipLaunchKernelGGL(k_unpad_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, add, dst, n, L, Lp);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

}  // namespace

int ms_conv1d_out_len(const ms_conv1d_desc* d) {
    ConvP p;
    return make_conv(d, &p) ? p.Lout : MS_ERR_INVALID_ARG;
}

int ms_convt1d_out_len(const ms_convt1d_desc* d) {
    ConvP p;
    return make_convt(d, &p) ? p.Lin : MS_ERR_INVALID_ARG;
}

}  // extern "C"

// ---- dispatch plans: which kernel a conv call runs
// Decided here and nowhere else.  A plan lists the routes of one call in the order they are tried, up to the first route that
// cannot pass the call on.  The entry points run the first route that takes the call; the queries read the same list: the
// kernel name is the first route's, the workspace covers every route in the list, a parts call is one launch unless its
// first route goes part by part.
namespace {

enum Kind {
    F_THIN_SHORT, F_SMALL, F_PAD4, F_MFMA, F_G4, F_G3, F_G, F_THIN, F_DIRECT,    // ms_conv1d_fwd
    D_PAD4, D_MFMA, D_G4, D_G3, D_G, D_THIN, D_DIRECT,                          // ms_conv1d_bwd_data (zero-padded geometry)
    W_THIN, W_SHORT, W_32, W_K5, W_ROWS, W_MFMA, W_G4, W_G3, W_G, W_DIRECT,     // ms_conv1d_bwd_weight
    TF_THIN, TF_LANES, TF_MFMA, TF_DIRECT,                                      // ms_convt1d_fwd (geometry: the mirrored conv)
    TD_MFMA, TD_CONV_MFMA, TD_CONV_DIRECT,                                      // ms_convt1d_bwd_data
    TW_THIN, TW_8, TW_2S, TW_MFMA, TW_CONV_MFMA, TW_CONV_DIRECT,                // ms_convt1d_bwd_weight
    P_DISC, P_G4, P_K5, P_K5_IMG, P_G3, P_EACH,                                 // ms_conv1d_parts_* (P_EACH: part by part)
};

// Route::declines, how a route may pass the call on (0: it takes every call that reaches it): its launcher may return
// MS_ERR_UNSUPPORTED (operand alignment and the like) / it is skipped when the workspace is short / not 16-byte aligned
enum : unsigned { UNSUPPORTED = 1, SHORT_WS = 2, ALIGNED_WS = 4 };

struct Route {
    Kind kind;
    unsigned declines;
    ConvP g;           // the geometry it runs on
    size_t ws;         // the workspace it needs
};

struct Plan {
    int n = 0;
    Route r[6];
    Plan& add(Kind k, const ConvP& g, size_t ws = 0, unsigned declines = 0) {
        r[n++] = Route{k, declines, g, ws};
        return *this;
    }
    size_t ws() const {
        size_t m = 0;
        for (int i = 0; i < n; ++i) m = r[i].ws > m ? r[i].ws : m;
        return m;
    }
};

// a single tensor as a table of one part (the 4 x 4 group kernels of gconv4.hip take 1 .. 3 parts)
ms_conv1d_parts one_part(const ConvP& p, const float* x = nullptr, float* y = nullptr, const float* gy = nullptr,
                         const float* y_act = nullptr, const float* gx_add = nullptr, float* gx = nullptr) {
    ms_conv1d_parts q{};
    q.count = 1;
    q.B[0] = p.B; q.Lin[0] = p.Lin;
    q.x[0] = x; q.y[0] = y; q.gy[0] = gy; q.y_act[0] = y_act; q.gx_add[0] = gx_add; q.gx[0] = gx;
    return q;
}

// residual, y_act: the call has them.  A route that cannot decline ends the plan (return).
Plan conv_plan(ConvP p, int which, bool residual, bool y_act) {
    Plan pl;
    const bool plain = !residual && !y_act;
    if (which == 0) {
        if (plain && mst_fwd_short_applicable(p)) return pl.add(F_THIN_SHORT, p);   // judge conv: a 12-MFLOP reduction, not a GEMM
        if (plain && mss_conv_applicable(p)) return pl.add(F_SMALL, p);            // a few dozen columns in the whole batch
        if (msm_fwd_applicable(p)) {
            if (plain && pad4_applicable(p)) {
                const ConvP q = pad4_conv(p);
                pl.add(F_PAD4, q, pad4_bytes(q, p.Cin) + pad4_bytes(q, p.Cout) + msm_fwd_ws(q), SHORT_WS | ALIGNED_WS);
            }
            return pl.add(F_MFMA, p, msm_fwd_ws(p));
        }
        if (plain && !p.in_act) {
            const ms_conv1d_parts q = one_part(p);
            if (msg4_parts_applicable(p, &q)) return pl.add(F_G4, p);
            if (msg3_fwd_applicable(p)) return pl.add(F_G3, p);
            if (msg_fwd_applicable(p)) return pl.add(F_G, p);
        }
        if (mst_fwd_applicable(p) && !y_act) return pl.add(F_THIN, p);
        return pl.add(F_DIRECT, p);
    }
    if (which == 1) {
        // reflection padding: the zero-padded backward gives the gradient of the in-range taps; the taps that read mirrored
        // samples are folded back onto their sources by an edge kernel behind (ms_conv1d_bwd_data)
        const bool reflect = p.pad_mode == MS_PAD_REFLECT;
        if (reflect && (p.stride != 1 || p.groups != 1)) return pl;
        p.pad_mode = MS_PAD_ZERO;
        if (msm_bwd_data_applicable(p)) {
            if (pad4_applicable(p)) {        // padded copies of gy (and y_act) and gx + the padded problem's own workspace
                const ConvP q = pad4_conv(p);
                pl.add(D_PAD4, q, pad4_bytes(q, p.Cout) * (y_act ? 2 : 1) + pad4_bytes(q, p.Cin) + msm_bwd_data_ws(q),
                       SHORT_WS | ALIGNED_WS);
            }
            return pl.add(D_MFMA, p, msm_bwd_data_ws(p));
        }
        const ms_conv1d_parts q = one_part(p);
        if (msg4_parts_applicable(p, &q)) return pl.add(D_G4, p);
        if (msg3_bwd_data_applicable(p)) return pl.add(D_G3, p);
        if (msg_bwd_data_applicable(p)) return pl.add(D_G, p);
        if (mst_bwd_data_applicable(p) && !reflect) return pl.add(D_THIN, p);
        return pl.add(D_DIRECT, p);
    }
    if (mst_bwd_weight_applicable(p)) return pl.add(W_THIN, p, mst_bwd_weight_ws(p));   // one-channel side: HBM-bound streams
    if (msws_applicable(p)) pl.add(W_SHORT, p, msws_ws(p), SHORT_WS | UNSUPPORTED);    // reflection-padded conv on short rows
    if (msw32_applicable(p)) pl.add(W_32, p, msw32_ws(p), UNSUPPORTED);               // 32 -> 32 k3 atoms: per-wave units
    if (msw5_applicable(p)) pl.add(W_K5, p, msw5_ws(p), SHORT_WS);                    // 1024 -> 1024 k5 on short rows
    if (msw_bwd_weight_applicable(p)) pl.add(W_ROWS, p, msw_bwd_weight_ws(p), UNSUPPORTED);   // dense stride-1: row tiles
    if (msm_bwd_weight_applicable(p)) return pl.add(W_MFMA, p, msm_bwd_weight_ws(p));
    if (!p.in_act) {
        const ms_conv1d_parts q = one_part(p);
        if (msg4_parts_applicable(p, &q)) return pl.add(W_G4, p);
        if (msg3_bwd_weight_applicable(p)) return pl.add(W_G3, p, msg_bwd_weight_ws(p));
        if (msg_bwd_weight_applicable(p)) return pl.add(W_G, p, msg_bwd_weight_ws(p));
    }
    return pl.add(W_DIRECT, p, msk_conv1d_bwd_weight_ws(p));
}

// p: the mirrored conv (make_convt)
Plan convt_plan(const ms_convt1d_desc* d, const ConvP& p, int which) {
    Plan pl;
    if (which == 0) {
        if (mst_convt1_applicable(p)) return pl.add(TF_THIN, p);            // one output channel: a stream
        if (mss_convt_applicable(d)) pl.add(TF_LANES, p, 0, UNSUPPORTED);    // inference batch: a weight stream
        // (its epilogue stores 8 / 16 bytes at a time: an output at a 4-byte address goes to the direct kernel)
        // (stride 4 ran without a workspace before its row-tile route existed: a call that brings none, or one off the 16-byte
        //  grid, keeps the direct kernel instead of being refused)
        if (msm_convt_fwd_applicable(p))
            pl.add(TF_MFMA, p, msm_convt_fwd_ws(p), UNSUPPORTED | (p.stride == 4 ? SHORT_WS | ALIGNED_WS : 0u));
        ConvP q = p;     // direct path: the loader modifier kind rides in q.act, the epilogue gets p.act
        q.act = p.in_act ? MS_MOD_LRELU_FWD : MS_ACT_NONE;
        return pl.add(TF_DIRECT, q);
    }
    if (which == 1) {
        if (msm_convt_bwd_applicable(p)) {
            if (p.stride != 4) return pl.add(TD_MFMA, p, msm_convt_bwd_data_ws(p));
            pl.add(TD_MFMA, p, msm_convt_bwd_data_ws(p), SHORT_WS | ALIGNED_WS);      // (as the forward: see above)
        }
        ConvP q = p;
        q.act = MS_ACT_NONE;
        if (msm_fwd_applicable(q)) {     // (this route's g.act is the kind of its activation OPERAND y_act: the conv has no epilogue)
            const size_t ws = msm_fwd_ws(q);
            q.act = p.act;
            return pl.add(TD_CONV_MFMA, q, ws);
        }
        return pl.add(TD_CONV_DIRECT, q);
    }
    // (every weight-gradient route also leaves the bias gradient's slice partials room at the workspace's tail;
    //  the first three routes exclude each other)
    const size_t tail = msk_channel_sum_ws(p.Cin) + 32;
    if (mst_convt1_applicable(p)) pl.add(TW_THIN, p, mst_convt1_wgrad_ws(p) + tail, SHORT_WS);
    if (mswt8_applicable(p)) pl.add(TW_8, p, mswt8_ws(p) + tail, SHORT_WS | UNSUPPORTED);
    if (mswt2s_applicable(p)) pl.add(TW_2S, p, mswt2s_ws(p) + tail, SHORT_WS | UNSUPPORTED);
    if (msm_convt_bwd_applicable(p)) return pl.add(TW_MFMA, p, msm_convt_bwd_weight_ws(p) + tail);
    if (msm_bwd_weight_applicable(p)) return pl.add(TW_CONV_MFMA, p, msm_bwd_weight_ws(p) + tail);
    return pl.add(TW_CONV_DIRECT, p, msk_conv1d_bwd_weight_ws(p) + tail);
}

bool parts_ok(const ms_conv1d_desc* d, const ms_conv1d_parts* parts, ConvP* c) {
    if (!d || !parts || parts->count < 1 || parts->count > MS_CONV_PARTS_MAX) return false;
    ms_conv1d_desc d0 = *d;
    for (int i = 0; i < parts->count; ++i) {
        d0.B = parts->B[i]; d0.Lin = parts->Lin[i];
        ConvP p;
        if (!make_conv(&d0, &p)) return false;
        if (i == 0) *c = p;
    }
    return true;
}

ms_conv1d_desc part_desc(const ms_conv1d_desc* d, const ms_conv1d_parts* parts, int i) {
    ms_conv1d_desc di = *d;
    di.B = parts->B[i]; di.Lin = parts->Lin[i];
    return di;
}

// c: the first part's conv (parts_ok); w, image: the call has the weights / a weight image
Plan parts_plan(const ms_conv1d_desc* d, const ConvP& c, const ms_conv1d_parts* parts, int which, bool w, bool image) {
    Plan pl;
    if (parts->count >= 2 && !c.in_act) {
        if (w && msd_parts_applicable(c, parts, which))
            return pl.add(P_DISC, c, which == 2 ? msd_parts_bwd_weight_ws(c, parts) : 0);
        if (w && msg4_parts_applicable(c, parts)) return pl.add(P_G4, c);
        if (which == 2 && msw5_parts_applicable(c, parts)) return pl.add(P_K5, c, msw5_parts_ws(c, parts));
        if (which < 2 && image && ms5_parts_applicable(c, parts, which == 1))
            return pl.add(P_K5_IMG, c, ms5_parts_ws(c, parts, which == 1));
        if (which == 0 && w && msg3_parts_fwd_applicable(c, parts)) return pl.add(P_G3, c);
        if (which == 1 && w && msg3_parts_bwd_data_applicable(c, parts)) return pl.add(P_G3, c);
        if (which == 2 && msg3_parts_bwd_weight_applicable(c, parts)) return pl.add(P_G3, c, msg3_parts_bwd_weight_ws(c, parts));
    }
    size_t n = 0;
    for (int i = 0; i < parts->count; ++i) {
        const ms_conv1d_desc di = part_desc(d, parts, i);
        const size_t m = image && which < 2 && ms_conv1d_img_bytes(&di) ? ms_conv1d_img_workspace_bytes(&di, which)
                                                                        : ms_conv1d_workspace_bytes(&di, which);
        if (m > n) n = m;
    }
    return pl.add(P_EACH, c, n);
}

const char* route_name(Kind k, const ConvP& g) {
    switch (k) {
        case F_THIN_SHORT: case F_THIN: return mst_fwd_name(g);
        case F_SMALL: return mss_conv_name(g);
        case F_PAD4: case F_MFMA: return msm_fwd_name(g);
        case TD_CONV_MFMA: { ConvP c = g; c.act = MS_ACT_NONE; return msm_fwd_name(c, g.act); }
        case F_G4: return msg4_parts_name(0);
        case F_G3: return msg3_fwd_name(g);
        case F_G: return msg_fwd_name(g);
        case F_DIRECT: case TD_CONV_DIRECT: return msk_conv1d_fwd_direct_name(g);
        case D_PAD4: case D_MFMA: return msm_bwd_data_name(g);
        case D_G4: return msg4_parts_name(1);
        case D_G3: return msg3_bwd_data_name(g);
        case D_G: return msg_bwd_data_name(g);
        case D_THIN: return mst_bwd_data_name(g);
        case D_DIRECT: case TF_DIRECT: return msk_conv1d_bwd_data_direct_name(g);
        case W_THIN: return mst_bwd_weight_name(g);
        case W_SHORT: return msws_name(g);
        case W_32: return msw32_name(g);
        case W_K5: return msw5_name(g);
        case W_ROWS: return msw_bwd_weight_name(g);
        case W_MFMA: case TW_CONV_MFMA: return msm_bwd_weight_name(g);
        case W_G4: return msg4_parts_name(2);
        case W_G3: return msg3_bwd_weight_name(g);
        case W_G: return msg_bwd_weight_name(g);
        case W_DIRECT: case TW_CONV_DIRECT: return msk_conv1d_bwd_weight_direct_name(g);
        case TF_THIN: return mst_convt1_fwd_name();
        case TF_LANES: return mss_convt_name(g.stride);
        case TF_MFMA: return msm_convt_fwd_name(g);
        case TD_MFMA: return msm_convt_bwd_data_name(g);
        case TW_THIN: return mst_convt1_wgrad_name();
        case TW_8: return mswt8_name(g);
        case TW_2S: return mswt2s_name(g);
        case TW_MFMA: return msm_convt_bwd_weight_name(g);
        default: return "";            // (the parts launchers note their own kernels)
    }
}

// Runs the plan: launch(kind, geometry) starts one route and returns its status.  In a profile session every route is noted before
// it launches; the launchers of the templated families then overwrite the note with their exact instantiation.
template <class Launch>
int run(const Plan& pl, const void* ws, size_t ws_bytes, Launch launch) {
    for (int i = 0; i < pl.n; ++i) {
        const Route& r = pl.r[i];
        if ((r.declines & SHORT_WS) && (!ws || ws_bytes < r.ws)) continue;
        if ((r.declines & ALIGNED_WS) && (((uintptr_t)ws) & 15)) continue;
        if (ms_prof_on()) ms_note_kernel(0, "%s", route_name(r.kind, r.g));
        const int rc = launch(r.kind, r.g);
        if (rc != MS_ERR_UNSUPPORTED || !(r.declines & UNSUPPORTED)) return rc;
    }
    return MS_ERR_UNSUPPORTED;           // (no route: the backward data of a strided or grouped reflection-padded conv)
}

}  // namespace

extern "C" {

int ms_conv1d_fwd(const ms_conv1d_desc* d, const float* x, const float* w, const float* bias,
                  const float* residual, float* y, float* y_act, void* workspace,
                  size_t workspace_bytes, ms_stream_t stream) {
    ConvP p;
    if (!make_conv(d, &p) || !x || !w || !y) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    // activation in front of the conv: applied to x on load (operand modifier "LeakyReLU of the value")
    const float* xa = p.in_act ? x : nullptr;
    const int xk = p.in_act ? MS_MOD_LRELU_FWD : 0;
    return run(conv_plan(p, 0, residual, y_act), workspace, workspace_bytes, [&](Kind k, const ConvP& g) {
        switch (k) {
            case F_THIN_SHORT: case F_THIN: return mst_conv1d_fwd(g, x, w, bias, residual, y, s);
            case F_SMALL: return mss_conv_fwd(g, x, w, bias, y, s);
            case F_PAD4: {                // x and y in rows padded to g.Lin, then the padded problem's own workspace
                const size_t xb = pad4_bytes(g, p.Cin), yb = pad4_bytes(g, p.Cout);
                float* xp = (float*)workspace;
                float* yp = (float*)((char*)workspace + xb);
                int rc = pad_rows(x, xp, (size_t)p.B * p.Cin, p.Lin, g.Lin, s);
                if (rc == MS_OK)
                    rc = msm_conv1d_fwd(g, xp, nullptr, 0, w, bias, nullptr, yp, nullptr, (char*)workspace + xb + yb,
                                        workspace_bytes - xb - yb, s);
                if (rc == MS_OK) rc = unpad_rows(yp, nullptr, y, (size_t)p.B * p.Cout, p.Lin, g.Lin, s);
                return rc;
            }
            case F_MFMA: return msm_conv1d_fwd(g, x, xa, xk, w, bias, residual, y, y_act, workspace, workspace_bytes, s);
            case F_G4: { const ms_conv1d_parts q = one_part(g, x, y); return msg4_parts_fwd(g, &q, w, bias, s); }
            case F_G3: return msg3_conv1d_fwd(g, x, w, bias, y, s);
            case F_G: return msg_conv1d_fwd(g, x, w, bias, y, s);
            default: return msk_conv1d_fwd_direct(g, x, xa, xk, w, bias, residual, y, y_act, s);
        }
    });
}

int ms_conv1d_bwd_data(const ms_conv1d_desc* d, const float* gy, const float* y_act,
                       const float* w, const float* gx_add, float* gx, void* workspace,
                       size_t workspace_bytes, ms_stream_t stream) {
    ConvP p;
    if (!make_conv(d, &p) || !gy || !w || !gx) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int rc = run(conv_plan(p, 1, false, y_act), workspace, workspace_bytes, [&](Kind k, const ConvP& g) {
        switch (k) {
            case D_PAD4: {                // gy (and y_act) and gx in rows padded to g.Lin, then the padded problem's workspace
                const size_t gb = pad4_bytes(g, p.Cout), xb = pad4_bytes(g, p.Cin);
                char* wsp = (char*)workspace;
                float* gp = (float*)wsp; wsp += gb;
                float* ap = nullptr;
                if (y_act) { ap = (float*)wsp; wsp += gb; }
                float* xp = (float*)wsp; wsp += xb;
                int rc = pad_rows(gy, gp, (size_t)p.B * p.Cout, p.Lin, g.Lin, s);
                if (rc == MS_OK && y_act) rc = pad_rows(y_act, ap, (size_t)p.B * p.Cout, p.Lin, g.Lin, s);
                if (rc == MS_OK)
                    rc = msm_conv1d_bwd_data(g, gp, ap, w, nullptr, xp, wsp, workspace_bytes - (size_t)(wsp - (char*)workspace), s);
                if (rc == MS_OK) rc = unpad_rows(xp, gx_add, gx, (size_t)p.B * p.Cin, p.Lin, g.Lin, s);
                return rc;
            }
            case D_MFMA: return msm_conv1d_bwd_data(g, gy, y_act, w, gx_add, gx, workspace, workspace_bytes, s);
            case D_G4: {
                const ms_conv1d_parts q = one_part(g, nullptr, nullptr, gy, y_act, gx_add, gx);
                return msg4_parts_bwd_data(g, &q, w, s);
            }
            case D_G3: return msg3_conv1d_bwd_data(g, gy, y_act, w, gx_add, gx, s);
            case D_G: return msg_conv1d_bwd_data(g, gy, y_act, w, gx_add, gx, s);
            case D_THIN: return mst_conv1d_bwd_data(g, gy, y_act, w, gx_add, gx, s);
            default: return msk_conv1d_bwd_data_direct(g, gy, y_act, w, nullptr, MS_ACT_NONE, gx_add, gx, s);
        }
    });
    if (rc != MS_OK || p.pad_mode != MS_PAD_REFLECT) return rc;
    p.pad_mode = MS_PAD_ZERO;
    return msk_reflect_fold_bwd(p, gy, y_act, w, gx, s);
}

int ms_conv1d_bwd_weight(const ms_conv1d_desc* d, const float* x, const float* gy,
                         const float* y_act, float* gw, float* gb, float beta, void* workspace,
                         size_t workspace_bytes, ms_stream_t stream) {
    ConvP p;
    if (!make_conv(d, &p) || !x || !gy || !gw) return MS_ERR_INVALID_ARG;
    if (beta != 0.f && beta != 1.f) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const float* xa = p.in_act ? x : nullptr;
    const int xk = p.in_act ? MS_MOD_LRELU_FWD : 0;
    return run(conv_plan(p, 2, false, false), workspace, workspace_bytes, [&](Kind k, const ConvP& g) {
        switch (k) {
            case W_THIN: return mst_conv1d_bwd_weight(g, x, gy, y_act, gw, gb, beta, workspace, workspace_bytes, s);
            case W_SHORT: return msws_bwd_weight(g, x, gy, y_act, gw, gb, beta, workspace, workspace_bytes, s);
            case W_32: return msw32_bwd_weight(g, x, gy, y_act, gw, gb, beta, workspace, workspace_bytes, s);
            case W_K5: return msw5_bwd_weight(g, x, gy, y_act, gw, gb, beta, workspace, workspace_bytes, s);
            case W_ROWS: return msw_conv1d_bwd_weight(g, x, gy, y_act, gw, gb, beta, workspace, workspace_bytes, s);
            case W_MFMA:
                return msm_conv1d_bwd_weight(g, x, xa, xk, gy, y_act, g.act, gw, gb, beta, workspace, workspace_bytes, s);
            case W_G4: {
                const ms_conv1d_parts q = one_part(g, x, nullptr, gy, y_act);
                return msg4_parts_bwd_weight(g, &q, gw, gb, beta, s);
            }
            case W_G3: return msg3_conv1d_bwd_weight(g, x, gy, y_act, gw, gb, beta, workspace, workspace_bytes, s);
            case W_G: return msg_conv1d_bwd_weight(g, x, gy, y_act, gw, gb, beta, workspace, workspace_bytes, s);
            default:
                return msk_conv1d_bwd_weight_direct(g, x, xa, xk, gy, y_act, g.act, gw, gb, beta, workspace, workspace_bytes, s);
        }
    });
}

// The query has no residual or saved activation; a call with them may reach routes a plain call does not: the workspace
// covers both.
size_t ms_conv1d_workspace_bytes(const ms_conv1d_desc* d, int which) {
    ConvP p;
    if (!make_conv(d, &p) || which < 0 || which > 2) return 0;
    const size_t a = conv_plan(p, which, false, false).ws(), b = conv_plan(p, which, true, true).ws();
    return a > b ? a : b;
}

const char* ms_conv1d_kernel_name(const ms_conv1d_desc* d, int which) {
    ConvP p;
    if (!make_conv(d, &p) || which < 0 || which > 2) return "";
    const Plan pl = conv_plan(p, which, false, false);
    return pl.n ? route_name(pl.r[0].kind, pl.r[0].g) : "";
}

// ---- one layer over several inputs (ms_conv1d_parts): a parts kernel where one applies, else part by part
int ms_conv1d_parts_launches(const ms_conv1d_desc* d, const ms_conv1d_parts* parts, int which, int with_image) {
    ConvP c;
    if (!parts_ok(d, parts, &c) || which < 0 || which > 2) return MS_ERR_INVALID_ARG;
    return parts_plan(d, c, parts, which, true, with_image != 0).r[0].kind == P_EACH ? parts->count : 1;
}

size_t ms_conv1d_parts_workspace_bytes(const ms_conv1d_desc* d, const ms_conv1d_parts* parts, int which, int with_image) {
    ConvP c;
    if (!parts_ok(d, parts, &c) || which < 0 || which > 2) return 0;
    return parts_plan(d, c, parts, which, true, with_image != 0).ws();
}

int ms_conv1d_parts_fwd(const ms_conv1d_desc* d, const ms_conv1d_parts* parts, const float* w, const float* bias,
                        const void* image, void* workspace, size_t workspace_bytes, ms_stream_t stream) {
    ConvP c;
    if (!parts_ok(d, parts, &c) || (!w && !image)) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    return run(parts_plan(d, c, parts, 0, w, image), workspace, workspace_bytes, [&](Kind k, const ConvP&) {
        switch (k) {
            case P_DISC: return msd_parts_fwd(c, parts, w, bias, s);
            case P_G4: return msg4_parts_fwd(c, parts, w, bias, s);
            case P_K5_IMG: return ms5_parts_fwd(c, parts, image, bias, workspace, workspace_bytes, s);
            case P_G3: return msg3_parts_fwd(c, parts, w, bias, s);
            default: break;
        }
        for (int i = 0; i < parts->count; ++i) {
            const ms_conv1d_desc di = part_desc(d, parts, i);
            int rc = MS_ERR_UNSUPPORTED;
            if (image && ms_conv1d_img_bytes(&di))
                rc = ms_conv1d_img_fwd(&di, parts->x[i], image, bias, parts->y[i], workspace, workspace_bytes, stream);
            else if (w)
                rc = ms_conv1d_fwd(&di, parts->x[i], w, bias, nullptr, parts->y[i], nullptr, workspace, workspace_bytes, stream);
            if (rc != MS_OK) return rc;
        }
        return (int)MS_OK;
    });
}

int ms_conv1d_parts_bwd_data(const ms_conv1d_desc* d, const ms_conv1d_parts* parts, const float* w, const void* image_bwd,
                             void* workspace, size_t workspace_bytes, ms_stream_t stream) {
    ConvP c;
    if (!parts_ok(d, parts, &c) || (!w && !image_bwd)) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    return run(parts_plan(d, c, parts, 1, w, image_bwd), workspace, workspace_bytes, [&](Kind k, const ConvP&) {
        switch (k) {
            case P_DISC: return msd_parts_bwd_data(c, parts, w, s);
            case P_G4: return msg4_parts_bwd_data(c, parts, w, s);
            case P_K5_IMG: return ms5_parts_bwd_data(c, parts, image_bwd, workspace, workspace_bytes, s);
            case P_G3: return msg3_parts_bwd_data(c, parts, w, s);
            default: break;
        }
        for (int i = 0; i < parts->count; ++i) {
            const ms_conv1d_desc di = part_desc(d, parts, i);
            const float* ya = d->act == MS_ACT_NONE ? nullptr : parts->y_act[i];
            int rc = MS_ERR_UNSUPPORTED;
            if (image_bwd && ms_conv1d_img_bytes(&di))
                rc = ms_conv1d_img_bwd_data(&di, parts->gy[i], ya, image_bwd, parts->gx_add[i], parts->gx[i], workspace,
                                            workspace_bytes, stream);
            else if (w)
                rc = ms_conv1d_bwd_data(&di, parts->gy[i], ya, w, parts->gx_add[i], parts->gx[i], workspace, workspace_bytes,
                                        stream);
            if (rc != MS_OK) return rc;
        }
        return (int)MS_OK;
    });
}

int ms_conv1d_parts_bwd_weight(const ms_conv1d_desc* d, const ms_conv1d_parts* parts, float* gw, float* gb, float beta,
                               void* workspace, size_t workspace_bytes, ms_stream_t stream) {
    ConvP c;
    if (!parts_ok(d, parts, &c) || !gw || (beta != 0.f && beta != 1.f)) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    return run(parts_plan(d, c, parts, 2, true, false), workspace, workspace_bytes, [&](Kind k, const ConvP&) {
        switch (k) {
            case P_DISC: return msd_parts_bwd_weight(c, parts, gw, gb, beta, workspace, workspace_bytes, s);
            case P_G4: return msg4_parts_bwd_weight(c, parts, gw, gb, beta, s);
            case P_K5: return msw5_parts_bwd_weight(c, parts, gw, gb, beta, workspace, workspace_bytes, s);
            case P_G3: return msg3_parts_bwd_weight(c, parts, gw, gb, beta, workspace, workspace_bytes, s);
            default: break;
        }
        for (int i = 0; i < parts->count; ++i) {         // the parts' gradients accumulate in order on the one stream
            const ms_conv1d_desc di = part_desc(d, parts, i);
            const float* ya = d->act == MS_ACT_NONE ? nullptr : parts->y_act[i];
            const int rc = ms_conv1d_bwd_weight(&di, parts->x[i], parts->gy[i], ya, gw, gb, i == 0 ? beta : 1.f, workspace,
                                                workspace_bytes, stream);
            if (rc != MS_OK) return rc;
        }
        return (int)MS_OK;
    });
}

static int multi_convs(const ms_wgrad_multi_desc* d, ConvP* cs) {
    if (!d || d->count <= 0 || d->count > MS_WGRAD_MULTI_MAX) return 0;
    for (int i = 0; i < d->count; ++i)
        if (!make_conv(&d->conv[i], &cs[i])) return 0;
    return d->count;
}

size_t ms_conv1d_bwd_weight_multi_workspace_bytes(const ms_wgrad_multi_desc* d) {
    ConvP cs[MS_WGRAD_MULTI_MAX];
    const int n = multi_convs(d, cs);
    size_t need = n ? msw_multi_ws(cs, n) : 0;
    if (n && msw32_multi_ws(cs, n) > need) need = msw32_multi_ws(cs, n);
    for (int i = 0; i < n; ++i) {
        const size_t one = ms_conv1d_workspace_bytes(&d->conv[i], 2);
        if (one > need) need = one;
    }
    return need;
}

int ms_conv1d_bwd_weight_multi(const ms_wgrad_multi_desc* d, void* workspace, size_t workspace_bytes,
                               ms_stream_t stream) {
    ConvP cs[MS_WGRAD_MULTI_MAX];
    const int n = multi_convs(d, cs);
    if (!n) return MS_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
        if (!d->x[i] || !d->gy[i] || !d->gw[i] || (d->beta[i] != 0.f && d->beta[i] != 1.f)) return MS_ERR_INVALID_ARG;
    // sign words in place of the activations: all entries or none, and only the two batched kernels read them
    int nsig = 0;
    for (int i = 0; i < n; ++i) nsig += d->y_signs[i] ? 1 : 0;
    if (nsig != 0 && nsig != n) return MS_ERR_INVALID_ARG;
    const float* ya[MS_WGRAD_MULTI_MAX];
    for (int i = 0; i < n; ++i) ya[i] = nsig ? reinterpret_cast<const float*>(d->y_signs[i]) : d->y_act[i];
    int rc = msw_conv1d_bwd_weight_multi(cs, n, d->x, d->gy, ya, d->gw, d->gb, d->beta, d->xmax, d->gmax, nsig ? 1 : 0, workspace,
                                         workspace_bytes, (hipStream_t)stream);
    if (rc != MS_ERR_UNSUPPORTED) return rc;
    rc = msw32_bwd_weight_multi(cs, n, d->x, d->gy, ya, d->gw, d->gb, d->beta, nsig ? 1 : 0, workspace, workspace_bytes,
                                (hipStream_t)stream);
    if (rc != MS_ERR_UNSUPPORTED) return rc;
    if (nsig) return MS_ERR_UNSUPPORTED;
    for (int i = 0; i < n; ++i) {       // geometry differs / unaligned operands: entry by entry
        const int r1 = ms_conv1d_bwd_weight(&d->conv[i], d->x[i], d->gy[i], d->y_act[i], d->gw[i], d->gb[i],
                                            d->beta[i], workspace, workspace_bytes, stream);
        if (r1 != MS_OK) return r1;
    }
    return MS_OK;
}

int ms_residual_stack_signs_supported(const ms_stack_desc* d) {
    if (!ms_switch_on("MSYNTH_ATOM_SIGNS")) return 0;            // tuning / test switch (0: the fp32 activations are saved)
    if (!d || d->count < 1 || d->count > MS_STACK_MAX || 2 * d->count > MS_WGRAD_MULTI_MAX) return 0;
    ConvP cs[MS_WGRAD_MULTI_MAX];
    int n = 0;
    for (int i = 0; i < d->count; ++i) {
        ms_atom_desc a = {d->B, d->C, d->L, d->dil[i], d->slope};
        if (!ms_residual_atom_sign_words(&a) || !ms_residual_atom_bwd_supported(&a)) return 0;
        // the two weight gradients of the atom: the dilation-1 conv (input t, gradient g masked by u) and the dilated one
        ms_conv1d_desc c1 = {d->B, d->C, d->L, d->C, 3, 1, 1, 1, 1, MS_PAD_ZERO, MS_ACT_LRELU, d->slope, MS_ACT_NONE};
        ms_conv1d_desc c0 = {d->B, d->C, d->L, d->C, 3, 1, d->dil[i], d->dil[i], 1, MS_PAD_ZERO, MS_ACT_LRELU, d->slope, MS_ACT_NONE};
        if (!make_conv(&c1, &cs[n++]) || !make_conv(&c0, &cs[n++])) return 0;
    }
    return (msw_multi_takes_signs(cs, n) || msw32_multi_takes_signs(cs, n)) ? 1 : 0;
}


// y = act(bias + conv_transpose(x, w)) == backward-data of the mirrored conv, with epilogue
int ms_convt1d_fwd(const ms_convt1d_desc* d, const float* x, const float* w, const float* bias,
                   float* y, void* workspace, size_t workspace_bytes, ms_stream_t stream) {
    ConvP p;
    if (!make_convt(d, &p) || !x || !w || !y) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    return run(convt_plan(d, p, 0), workspace, workspace_bytes, [&](Kind k, const ConvP& g) {
        switch (k) {
            case TF_THIN: return mst_convt1_fwd(g, x, w, bias, y, s);
            case TF_LANES: return mss_convt_fwd(d, x, w, bias, y, s);
            case TF_MFMA: return msm_convt1d_fwd(g, x, w, bias, y, workspace, workspace_bytes, s);
            default: return msk_conv1d_bwd_data_direct(g, x, p.in_act ? x : nullptr, w, bias, p.act, nullptr, y, s);
        }
    });
}

// gx = conv(gy * act'(y_act), w) with the mirrored conv geometry (no bias / activation)
int ms_convt1d_bwd_data(const ms_convt1d_desc* d, const float* gy, const float* y_act,
                        const float* w, float* gx, void* workspace, size_t workspace_bytes,
                        ms_stream_t stream) {
    ConvP p;
    if (!make_convt(d, &p) || !gy || !w || !gx) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    return run(convt_plan(d, p, 1), workspace, workspace_bytes, [&](Kind k, const ConvP& g) {
        switch (k) {
            case TD_MFMA: return msm_convt1d_bwd_data(g, gy, y_act, w, gx, workspace, workspace_bytes, s);
            case TD_CONV_MFMA: {
                ConvP c = g;
                c.act = MS_ACT_NONE;
                return msm_conv1d_fwd(c, gy, y_act, g.act, w, nullptr, nullptr, gx, nullptr, workspace, workspace_bytes, s);
            }
            default: return msk_conv1d_fwd_direct(g, gy, y_act, p.act, w, nullptr, nullptr, gx, nullptr, s);
        }
    });
}

// gw[ci_T, co_T, k] = sum x[b,ci_T,i] * gp[b,co_T,i*stride - pad + k]: the mirrored conv's weight
// grad with its "input" = gp (activation modifier on that side) and its "output grad" = x.
int ms_convt1d_bwd_weight(const ms_convt1d_desc* d, const float* x, const float* gy,
                          const float* y_act, float* gw, float* gb, float beta, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream) {
    ConvP p;
    if (!make_convt(d, &p) || !x || !gy || !gw) return MS_ERR_INVALID_ARG;
    if (beta != 0.f && beta != 1.f) return MS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const float* xa = p.in_act ? x : nullptr;
    const int xk = p.in_act ? MS_MOD_LRELU_FWD : 0;
    const int rc = run(convt_plan(d, p, 2), workspace, workspace_bytes, [&](Kind k, const ConvP& g) {
        switch (k) {
            case TW_THIN: return mst_convt1_bwd_weight(p, x, gy, y_act, gw, beta, workspace, workspace_bytes, s);
            case TW_8: return mswt8_bwd_weight(p, x, gy, y_act, gw, beta, workspace, workspace_bytes, s);
            case TW_2S: return mswt2s_bwd_weight(p, x, gy, y_act, gw, beta, workspace, workspace_bytes, s);
            case TW_MFMA: return msm_convt1d_bwd_weight(p, x, gy, y_act, gw, beta, workspace, workspace_bytes, s);
            case TW_CONV_MFMA:
                return msm_conv1d_bwd_weight(p, gy, y_act, p.act, x, xa, xk, gw, nullptr, beta, workspace, workspace_bytes, s);
            default:
                return msk_conv1d_bwd_weight_direct(p, gy, y_act, p.act, x, xa, xk, gw, nullptr, beta, workspace,
                                                    workspace_bytes, s);
        }
    });
    if (rc != MS_OK) return rc;
    if (gb) {   // bias grad: the slice partials live at the tail of the workspace
        const size_t tail = msk_channel_sum_ws(p.Cin);
        if (!workspace || workspace_bytes < tail) return MS_ERR_WORKSPACE;
        char* wtail = (char*)workspace + (workspace_bytes - tail);
        wtail -= ((uintptr_t)wtail) & 15;
        if (wtail < (char*)workspace) return MS_ERR_WORKSPACE;
        return msk_channel_sum(gy, y_act, p.act, p.slope, p.B, p.Cin, p.Lin, gb, beta, wtail, tail, s);
    }
    return MS_OK;
}

size_t ms_convt1d_workspace_bytes(const ms_convt1d_desc* d, int which) {
    ConvP p;
    return make_convt(d, &p) && which >= 0 && which <= 2 ? convt_plan(d, p, which).ws() : 0;
}

const char* ms_convt1d_kernel_name(const ms_convt1d_desc* d, int which) {
    ConvP p;
    if (!make_convt(d, &p) || which < 0 || which > 2) return "";
    const Plan pl = convt_plan(d, p, which);
    return route_name(pl.r[0].kind, pl.r[0].g);
}

}  // extern "C"
