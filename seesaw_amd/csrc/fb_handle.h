// fb_handle.h -- the feedback engine's handle and the host functions its sources share: feedback.hip (the C entry
// points), feedback_eval.hip, feedback_fit_wg.hip and feedback_lbfgs.hip.  The arithmetic is fb_math.h's.
#pragma once
#include <string>
#include <vector>

#include "fb_math.h"

constexpr int FIT_WG_MAX_ROWS = 1024;  // labelled rows one fit workgroup reaches (feedback_fit_wg.hip)
constexpr int FIT_HISTORY = 100;       // L-BFGS history entries (torch's default)

// the arguments of one fit workgroup (k_fb_fit_wg by value, k_fb_fit_wg_batch one table entry a block)
struct FitWgArgs {
    const float *X, *y, *coef;   // [n, dim] centred rows, targets, per-item coefficients
    const float *qhat, *xlx;     // or null
    const float *w0_or_null;     // initial parameters when they do not fit the argument segment
    float *hist_dirs, *hist_stps;  // [FIT_HISTORY, 1024] (rows padded: the driving wave loads without bounds checks)
    float *out_w;                // mapped host memory: [dim + 1]
    double *out_loss;            // mapped host
    int *out_counts;             // mapped host: iterations, evaluations, status (0 ok, 1 loss diverged), diagnostics
    unsigned *done_flag;
    unsigned seqno;
    int n, dim, P;               // P = trainable parameters (dim or dim + 1)
    int label_mode;              // 0 elementwise BCE, 1 pairwise hinge, 2 pairwise logistic, 3 identically zero
    int onepass;                 // fit_eval_onepass instead of the logits / labels / gradient phases (same bits)
    float pw, margin;
    int max_iter;
    float lr;
    ssw::FbObjDev obj;
    // k_fb_fit2_wg (two outputs): y = two target planes `plane2` floats apart, coef = the sample weights, dim2 = the
    // rows' width; dim = 2 dim2 - 1 and P = 2 dim2 are what the driver step sees (2 dim2 parameters, no unused slot)
    int dim2, plane2;
};

struct ssw_fb {
    int device = 0;
    int dim = 0;
    int64_t n = 0, cap = 0;
    float *X = nullptr;        // [cap, dim] centred rows
    float *mu = nullptr;       // [dim]
    float *y = nullptr, *coef = nullptr, *z = nullptr, *r = nullptr;  // [cap]
    double *item = nullptr;    // [cap] per-item label losses (f64)
    double *loss_dev = nullptr, *loss_host = nullptr;  // total loss in f64
    int64_t *rows = nullptr;   // gather staging
    float *partial = nullptr;  // [nslabs(cap), dim]
    float *gsum = nullptr;     // [1024] ordered column sums of the slab partials (k_fb_slabsum, sets of >= 2048 rows)
    float *rankg = nullptr;    // [cap] net position changes of the rank objective (SSW_FB_RANKREG)
    // two-output objective (ssw_fb_*2): planes of cap floats / [2][nslabs(cap)][dim] partial gradients
    float *y2 = nullptr, *sw2 = nullptr, *z2 = nullptr, *r2 = nullptr, *itemv = nullptr, *itemh = nullptr;
    float *partial2 = nullptr, *nw2 = nullptr;
    float *w2 = nullptr;       // [2 dim + 2] raw weights of a device evaluation, then the two row norms (fb_eval2_dev)
    float *out2_host = nullptr, *out2_host_dev = nullptr;  // mapped pinned [2 + 2 dim]
    int64_t cap2 = 0;
    bool has_targets2 = false;
    double *colsum = nullptr;  // [cap / FB_CENTER_ROWS, dim] block sums of the centring step
    float *w = nullptr;        // [dim + 1]
    float *qhat = nullptr;     // [dim]
    float *xlx = nullptr;      // [dim, dim]
    bool has_q = false, has_xlx = false;
    float *out = nullptr;      // device [1 + dim + 1 + 4]
    float *out_host = nullptr;  // pinned mirror
    float *out_host_dev = nullptr;     // the same memory through the device's address space
    double *loss_host_dev = nullptr;
    unsigned *flag_host = nullptr, *flag_host_dev = nullptr;  // mapped pinned completion word of the closure evaluation
    unsigned seqno = 0;
    float *w_host = nullptr;    // pinned staging
    hipStream_t stream = nullptr;
    // targets (host copies, for the objective set-up)
    std::vector<float> y_host, sw_host;
    // pinned staging of the per-round uploads (row ids, targets, query): queued on the stream without a wait -- the fit
    // that follows is stream-ordered behind them (a refine spent ~35 us in three synchronisations here)
    ssw::PinnedStage rows_stage, y_stage, q_stage, coef_stage, th_stage, drawn_stage;
    int64_t *th = nullptr, *drawn = nullptr;  // ssw_fb_set_pseudo_sample: labelled[j] - j, the draw
    int64_t th_cap = 0, drawn_cap = 0;
    bool targets_on_device = false;           // the targets were formed on the device: y_host holds only the labelled part
    std::vector<float> qhat_host;  // the normalised query (host copy, for the two-output objective's host part)
    // diagnostics of the last fit
    int last_iters = 0, last_evals = 0;
    float rank_factor = 0.f;   // 1 / total_pairs of the installed targets (SSW_FB_RANKREG)
    float *hist = nullptr;     // [2, FIT_HISTORY, 1024] L-BFGS history of the single-launch fit
    bool last_fit_on_device = false;
    // ssw_fb_fit_batch: the engine of a launch's first slot lends the argument and start-vector tables
    FitWgArgs *batch_tab = nullptr;  // [batch_cap]
    float *batch_w = nullptr;        // [batch_cap, dim + 1]
    int batch_cap = 0;
    ssw::PinnedStage batch_tab_stage, batch_w_stage;
    hipEvent_t batch_ev = nullptr;   // "this engine's uploads are queued", for the launch stream to wait on
    std::string batch_error;         // this engine's slot of the last batch: the message ssw_fb_fit would have set, or empty
};

#pragma GCC visibility push(hidden)  // shared between the library's own sources, not exported from it
namespace ssw {

// what the host L-BFGS evaluates: f(x + t d) and its gradient, through fb_eval or (two) fb_eval2
struct Evaluator {
    ssw_fb *fb;
    const ssw_fb_objective *o;
    FbObjDev dev;
    float pw;
    bool pairwise_active;
    int P;
    bool two = false;            // the two-output objective (fb_eval2) instead of fb_eval
    bool two_dev = false;        // ... evaluated entirely on the device (fb_eval2_dev)
    float l_norm2 = 0.f, l_query2 = 0.f;
    ssw_status status = SSW_OK;
    bool eval(const std::vector<float> &x, double t, const std::vector<float> &d, double *f, std::vector<float> *g);
};

inline int fb_fit_params(const ssw_fb *fb, const ssw_fb_objective *obj) {
    return fb->dim + ((obj->kind == SSW_FB_LOGREG && obj->fit_intercept) ? 1 : 0);
}

// feedback_eval.hip: device buffers, data preparation, one closure evaluation
ssw_status fb_reserve(ssw_fb *fb, int64_t n);
ssw_status fb2_reserve(ssw_fb *fb);
ssw_status fb_center(ssw_fb *fb, int center);
ssw_status fb_prepare(ssw_fb *fb, const ssw_fb_objective *o, FbObjDev *dev, float *pw_out, bool *pairwise_active);
ssw_status fb_eval(ssw_fb *fb, const ssw_fb_objective *o, const FbObjDev &dev, float pw, bool pairwise_active, int P);
ssw_status fb_eval2(ssw_fb *fb, float l_norm, float l_query, float *parts5);
ssw_status fb_eval2_dev(ssw_fb *fb, float l_norm, float l_query, float *parts5);  // the same with no host arithmetic
ssw_status fb2_dev_reserve(ssw_fb *fb);
void launch_fb_logits(ssw_fb *fb, int has_bias);  // k_fb_logits: fb->z = fb->X fb->w (+ b)
void launch_fb_pairwise(int logistic, const float *z, const float *y, const float *coef, float margin, int n,
                        double *item_loss, float *r, hipStream_t stream);
void launch_fb_pseudo_rows(ssw_fb *fb, int64_t n_lab, int64_t n_drawn, const double *dev_scores, int64_t n_scores);

// feedback_fit_wg.hip: the one-launch fit's host side
bool fb_fit_wg_eligible(const ssw_fb *fb, const ssw_fb_objective *obj);
void fb_fit_wg_fill(ssw_fb *fb, const ssw_fb_objective *obj, const FbObjDev &dev, float pw, bool pairwise_active,
                    int max_iter, float lr, FitWgArgs *out);
ssw_status fb_fit_wg_launch(ssw_fb *fb, const FitWgArgs &a, const FbW &w0v);
ssw_status fb_fit_wg_launch_batch(ssw_fb *lead, const FitWgArgs *tab, int nwg);
bool fb_fit_wg_spin(const ssw_fb *fb, unsigned want);
ssw_status fb_fit_wg_collect(ssw_fb *fb, int P, float *w_inout, int32_t *out_iters, int32_t *out_evals,
                             float *out_final_loss);
ssw_status fb_batch_reserve(ssw_fb *fb, int nfit);
bool fb_fit2_wg_eligible(const ssw_fb *fb);
void fb_fit2_wg_fill(ssw_fb *fb, float l_norm, float l_query, int max_iter, float lr, const float *w0_dev, FitWgArgs *out);
ssw_status fb_fit2_wg_launch(ssw_fb *lead, const FitWgArgs *tab_host, int nwg);  // nwg = 1: tab_host[0] by value

// feedback_lbfgs.hip: torch.optim.LBFGS.step(closure) driven from the host
extern double g_fit_eval_s;  // diagnostic (SSW_FB_TIMING): seconds of the last fit spent inside closure evaluations
ssw_status lbfgs_host(Evaluator &E, std::vector<float> &x, int zero_slot, int max_iter, float lr, int *n_iter_out,
                      double *loss_out);

}  // namespace ssw
#pragma GCC visibility pop
