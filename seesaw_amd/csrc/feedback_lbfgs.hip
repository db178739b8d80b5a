// feedback_lbfgs.hip -- the feedback engine's host-driven fit: L-BFGS with strong-Wolfe line search around one closure
// evaluation at a time (fb_eval / fb_eval2, feedback_eval.hip).  The engine's overview is in feedback.hip.
// Restatement of the algorithm torch.optim.LBFGS implements (minFunc's lbfgs / lswolfe with
// cubic interpolation; defaults history 100, tolerance_grad 1e-7, tolerance_change 1e-9,
// c1 1e-4, c2 0.9, max_ls 25), which is what the reference drives through
// BasicTrainer.fit -> opt.step(closure) (basic_trainer.py:59-63).
// Host code only, and still compiled with -ffp-contract=off (Makefile): this f32 / f64 arithmetic is the state
// machine fit_driver_step (feedback_fit_wg.hip) walks on the device, operation for operation, and the two must round
// alike -- a contracted a * b + c here changes the fit's bits without failing the build.  The sums and the
// interpolation both sides share are fb_math.h's (wave_sum_host, cubic_interpolate_dev).
#include <chrono>
#include <cmath>
#include <vector>

#include "fb_handle.h"

namespace ssw {

double g_fit_eval_s = 0;

// f(x + t d) and its gradient
bool Evaluator::eval(const std::vector<float> &x, double t, const std::vector<float> &d, double *f, std::vector<float> *g) {
    for (int i = 0; i < P; ++i) fb->w_host[i] = x[i] + (float)t * d[i];
    const auto t0 = std::chrono::steady_clock::now();
    status = two ? (two_dev ? fb_eval2_dev(fb, l_norm2, l_query2, nullptr) : fb_eval2(fb, l_norm2, l_query2, nullptr))
                 : fb_eval(fb, o, dev, pw, pairwise_active, P);
    g_fit_eval_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (status != SSW_OK) return false;
    *f = fb->loss_host[0];
    g->assign(fb->out_host + 1, fb->out_host + 1 + P);
    if (!std::isfinite(*f)) {
        set_error("feedback: loss diverged (%g) -- regression training failed with a nan", *f);
        status = SSW_ERR_NUMERIC;  // logistic_regression.py:398-401
        return false;
    }
    return true;
}

namespace {

typedef std::vector<float> Vec;

// dot products in the association of fit_driver_step's vdot: per-lane products, then wave_sum_f's network
double vdot(const Vec &a, const Vec &b) {
    float p[1032];
    for (size_t i = 0; i < a.size(); ++i) p[i] = a[i] * b[i];
    return (double)wave_sum_host(p, a.size());
}
double vabsmax(const Vec &a) {
    float m = 0.f;
    for (float v : a) m = std::fmax(m, std::fabs(v));
    return m;
}

// returns false on evaluator failure
bool strong_wolfe(Evaluator &E, const Vec &x, double t, const Vec &d, double f, const Vec &g, double gtd,
                  double *f_out, Vec *g_out, double *t_out, int *evals, double c1 = 1e-4, double c2 = 0.9,
                  double tol_change = 1e-9, int max_ls = 25) {
    const double d_norm = vabsmax(d);
    double f_new;
    Vec g_new;
    if (!E.eval(x, t, d, &f_new, &g_new)) return false;
    int ls_evals = 1;
    double gtd_new = vdot(g_new, d);
    double t_prev = 0, f_prev = f, gtd_prev = gtd;
    Vec g_prev = g;
    bool done = false;
    int ls_iter = 0;
    double br[2] = {0, 0}, br_f[2] = {0, 0}, br_gtd[2] = {0, 0};
    Vec br_g[2];
    int nbr = 0;
    while (ls_iter < max_ls) {
        if (f_new > (f + c1 * t * gtd) || (ls_iter > 1 && f_new >= f_prev)) {
            br[0] = t_prev; br[1] = t; br_f[0] = f_prev; br_f[1] = f_new;
            br_g[0] = g_prev; br_g[1] = g_new; br_gtd[0] = gtd_prev; br_gtd[1] = gtd_new; nbr = 2;
            break;
        }
        if (std::fabs(gtd_new) <= -c2 * gtd) {
            br[0] = t; br_f[0] = f_new; br_g[0] = g_new; nbr = 1;
            done = true;
            break;
        }
        if (gtd_new >= 0) {
            br[0] = t_prev; br[1] = t; br_f[0] = f_prev; br_f[1] = f_new;
            br_g[0] = g_prev; br_g[1] = g_new; br_gtd[0] = gtd_prev; br_gtd[1] = gtd_new; nbr = 2;
            break;
        }
        const double min_step = t + 0.01 * (t - t_prev), max_step = t * 10;
        const double tmp = t;
        t = cubic_interpolate_dev(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, true, min_step, max_step);
        t_prev = tmp; f_prev = f_new; g_prev = g_new; gtd_prev = gtd_new;
        if (!E.eval(x, t, d, &f_new, &g_new)) return false;
        ls_evals++;
        gtd_new = vdot(g_new, d);
        ls_iter++;
    }
    if (ls_iter == max_ls) {
        br[0] = 0; br[1] = t; br_f[0] = f; br_f[1] = f_new; br_g[0] = g; br_g[1] = g_new; nbr = 2;
        br_gtd[0] = gtd; br_gtd[1] = gtd_new;
    }
    bool insuf = false;
    int low = 0, high = 0;
    if (nbr == 2) {
        low = br_f[0] <= br_f[1] ? 0 : 1;
        high = 1 - low;
    }
    while (!done && ls_iter < max_ls) {
        if (std::fabs(br[1] - br[0]) * d_norm < tol_change) break;
        t = cubic_interpolate_dev(br[0], br_f[0], br_gtd[0], br[1], br_f[1], br_gtd[1], false, 0, 0);
        const double bmax = std::fmax(br[0], br[1]), bmin = std::fmin(br[0], br[1]);
        const double eps = 0.1 * (bmax - bmin);
        if (std::fmin(bmax - t, t - bmin) < eps) {
            if (insuf || t >= bmax || t <= bmin) {
                t = (std::fabs(t - bmax) < std::fabs(t - bmin)) ? bmax - eps : bmin + eps;
                insuf = false;
            } else {
                insuf = true;
            }
        } else {
            insuf = false;
        }
        if (!E.eval(x, t, d, &f_new, &g_new)) return false;
        ls_evals++;
        gtd_new = vdot(g_new, d);
        ls_iter++;
        if (f_new > (f + c1 * t * gtd) || f_new >= br_f[low]) {
            br[high] = t; br_f[high] = f_new; br_g[high] = g_new; br_gtd[high] = gtd_new;
            low = br_f[0] <= br_f[1] ? 0 : 1;
            high = 1 - low;
        } else {
            if (std::fabs(gtd_new) <= -c2 * gtd) {
                done = true;
            } else if (gtd_new * (br[high] - br[low]) >= 0) {
                br[high] = br[low]; br_f[high] = br_f[low]; br_g[high] = br_g[low]; br_gtd[high] = br_gtd[low];
            }
            br[low] = t; br_f[low] = f_new; br_g[low] = g_new; br_gtd[low] = gtd_new;
        }
    }
    *t_out = br[low];
    *f_out = br_f[low];
    *g_out = br_g[low];
    *evals = ls_evals;
    return true;
}

}  // namespace

// torch.optim.LBFGS.step(closure) driven from the host: x [E.P] in/out; `zero_slot` (or -1) is a parameter slot the
// objective does not use (the bias of a fit without intercept) whose gradient is held at zero
ssw_status lbfgs_host(Evaluator &E, Vec &x, int zero_slot, int max_iter, float lr, int *n_iter_out, double *loss_out) {
    const int history = 100;
    const double tol_grad = 1e-7, tol_change = 1e-9;
    const int max_eval = max_iter * 5 / 4;
    Vec d(E.P, 0.f), g, prev_g, zero(E.P, 0.f);
    double loss;
    if (!E.eval(x, 0.0, zero, &loss, &g)) return E.status;
    if (zero_slot >= 0) g[zero_slot] = 0.f;
    int current_evals = 1, n_iter = 0;
    double t = 0, prev_loss = loss, H_diag = 1.0;
    std::vector<Vec> old_dirs, old_stps;
    std::vector<double> ro;
    bool opt_cond = vabsmax(g) <= tol_grad;
    while (!opt_cond && n_iter < max_iter) {
        n_iter++;
        if (n_iter == 1) {
            for (int i = 0; i < E.P; ++i) d[i] = -g[i];
            H_diag = 1.0;
        } else {
            Vec yv(E.P), sv(E.P);
            for (int i = 0; i < E.P; ++i) {
                yv[i] = g[i] - prev_g[i];
                sv[i] = d[i] * (float)t;
            }
            const double ys = vdot(yv, sv);
            if (ys > 1e-10) {
                if ((int)old_dirs.size() == history) {
                    old_dirs.erase(old_dirs.begin());
                    old_stps.erase(old_stps.begin());
                    ro.erase(ro.begin());
                }
                old_dirs.push_back(yv);
                old_stps.push_back(sv);
                ro.push_back(1.0 / ys);
                H_diag = ys / vdot(yv, yv);
            }
            const int m = (int)old_dirs.size();
            std::vector<double> al((size_t)m);
            Vec q(E.P);
            for (int i = 0; i < E.P; ++i) q[i] = -g[i];
            for (int i = m - 1; i >= 0; --i) {
                al[(size_t)i] = vdot(old_stps[(size_t)i], q) * ro[(size_t)i];
                for (int j = 0; j < E.P; ++j) q[j] -= (float)al[(size_t)i] * old_dirs[(size_t)i][j];
            }
            for (int j = 0; j < E.P; ++j) d[j] = q[j] * (float)H_diag;
            for (int i = 0; i < m; ++i) {
                const double be = vdot(old_dirs[(size_t)i], d) * ro[(size_t)i];
                for (int j = 0; j < E.P; ++j) d[j] += (float)(al[(size_t)i] - be) * old_stps[(size_t)i][j];
            }
        }
        prev_g = g;
        prev_loss = loss;
        if (n_iter == 1) {
            double pa[1032];
            for (size_t i = 0; i < g.size(); ++i) pa[i] = (double)std::fabs(g[i]);
            const double gs = wave_sum_host(pa, g.size());
            t = std::fmin(1.0, 1.0 / gs) * lr;
        } else {
            t = lr;
        }
        const double gtd = vdot(g, d);
        if (gtd > -tol_change) break;
        double f_new, t_new;
        Vec g_new;
        int ls_evals = 0;
        if (!strong_wolfe(E, x, t, d, loss, g, gtd, &f_new, &g_new, &t_new, &ls_evals)) return E.status;
        loss = f_new;
        g = g_new;
        if (zero_slot >= 0) g[zero_slot] = 0.f;
        t = t_new;
        for (int i = 0; i < E.P; ++i) x[i] += (float)t * d[i];
        opt_cond = vabsmax(g) <= tol_grad;
        current_evals += ls_evals;
        if (n_iter == max_iter) break;
        if (current_evals >= max_eval) break;
        if (opt_cond) break;
        double dm = 0;
        for (int i = 0; i < E.P; ++i) dm = std::fmax(dm, std::fabs((double)d[i] * t));
        if (dm <= tol_change) break;
        if (std::fabs(loss - prev_loss) < tol_change) break;
    }
    *n_iter_out = n_iter;
    *loss_out = loss;
    return SSW_OK;
}

}  // namespace ssw
