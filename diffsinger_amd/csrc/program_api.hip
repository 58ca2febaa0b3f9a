// libdsdenoise, the sampler programs built in the library: dsd_ddpm_tables_fill, dsd_program_build / dsd_program_free,
// dsd_onnx_ddpm_plan.  Host code only - no kernel, no HIP call, no HIP header - so the same file also compiles with a
// plain host C++ compiler (tools/harness/program_harness.cpp builds it that way, under the sanitizers).
//
// This is diffsinger_amd/schedule.py restated in C++.  schedule.py stays the yardstick: tests/test_cprogram_host.py holds
// every program built here against the one schedule.py builds.  The arithmetic keeps schedule.py's three regimes apart:
//   fp32   where schedule.py uses fp32 torch scalars (the reference's own arithmetic: lambda and sigma are
//          ill-conditioned near t -> 0, so "the same formula in double" gives another trajectory): every operation is
//          one fp32 operation here, in the same order; contraction into FMAs is switched off for the file, and the one
//          place where torch itself contracts (linspace) says so;
//   Lin    the linear expressions over {model output, buffers, noise}: Python floats, so doubles, one operation per
//          Python operation - the class below mirrors schedule.Lin operator by operator;
//   double the DDPM tables, rounded to fp32 once.
// expf / logf / expm1f come from the C math library where schedule.py has torch's (SLEEF) and numpy's: those results may
// differ in the last place, which is why the programs of the ancestral sampler, DPM-Solver++ and UniPC are not promised
// bit-equal to schedule.py's (DESIGN.md section 5 has the measured differences).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <utility>
#include <vector>

#include "../../include/dsdenoise.h"

struct dsd_handle;
namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);
}  // namespace dsd
using dsd::fail;

namespace {

// schedule.DDPMTables.NAMES, in that order: the DSD_DDPM_TABLES rows of `tables`
enum { TB_BETAS = 0, TB_AC, TB_AC_PREV, TB_SQRT_AC, TB_SQRT_1M_AC, TB_LOG_1M_AC, TB_SQRT_RECIP_AC, TB_SQRT_RECIPM1_AC,
       TB_POST_VAR, TB_POST_LOGVAR, TB_POST_C1, TB_POST_C2 };

// ------------------------------------------------------------------------------------------
// schedule.Lin: {source: coefficient} with Python-float arithmetic
// ------------------------------------------------------------------------------------------
struct Lin {
    std::vector<std::pair<int, double>> c;
    Lin() {}
    Lin(int src, double coef) { c.emplace_back(src, coef); }
    Lin operator+(const Lin& o) const {
        Lin r = *this;
        for (const auto& kv : o.c) {
            bool found = false;
            for (auto& rv : r.c)
                if (rv.first == kv.first) {
                    rv.second = rv.second + kv.second;
                    found = true;
                    break;
                }
            if (!found) r.c.emplace_back(kv.first, 0.0 + kv.second);       // r.get(k, 0.0) + v
        }
        return r;
    }
    Lin operator*(double s) const {
        Lin r = *this;
        for (auto& rv : r.c) rv.second = rv.second * s;
        return r;
    }
    Lin operator-(const Lin& o) const { return *this + (o * -1.0); }
    Lin operator/(double s) const { return *this * (1.0 / s); }
};
inline Lin of(int src, double coef = 1.0) { return Lin(src, coef); }
inline int noise_src(int k) { return DSD_SRC_NOISE_BASE - k; }

// Lin.terms(): the model output first, then buffers, then noise; exact zeros dropped
bool term_before(int a, int b) {
    const int ka[3] = {a != DSD_SRC_MODEL, a < 0, a < 0 ? -a : a}, kb[3] = {b != DSD_SRC_MODEL, b < 0, b < 0 ? -b : b};
    return std::lexicographical_compare(ka, ka + 3, kb, kb + 3);
}

struct Builder {
    std::vector<dsd_eval> evals;
    int err = 0;        // 1: too many terms, 2: too many outputs
    void begin(int x_buf, float t) {
        dsd_eval e;
        memset(&e, 0, sizeof(e));
        e.x_buf = x_buf;
        e.t = t;
        evals.push_back(e);
    }
    void emit(int dst, const Lin& expr) {
        dsd_eval& e = evals.back();
        if (e.n_out >= DSD_MAX_OUT) {
            err = 2;
            return;
        }
        std::vector<std::pair<int, double>> ks = expr.c;
        std::sort(ks.begin(), ks.end(), [](const std::pair<int, double>& a, const std::pair<int, double>& b) {
            return term_before(a.first, b.first);
        });
        dsd_lincomb& lc = e.out[e.n_out];
        lc.dst = dst;
        int n = 0;
        for (const auto& kv : ks) {
            if (kv.second == 0.0) continue;
            if (n >= DSD_MAX_TERMS) {
                err = 1;
                return;
            }
            lc.terms[n].src = kv.first;
            lc.terms[n].coef = (float)kv.second;
            ++n;
        }
        if (n == 0 && !ks.empty()) {         // every coefficient is zero: one zero term keeps the output defined
            lc.terms[0].src = ks[0].first;
            lc.terms[0].coef = 0.0f;
            n = 1;
        }
        lc.n_terms = n;
        ++e.n_out;
    }
};

// ------------------------------------------------------------------------------------------
// DDPM tables in double (schedule.linear_beta_schedule / cosine_beta_schedule / DDPMTables.__init__)
// ------------------------------------------------------------------------------------------
// numpy.linspace(start, stop, num), endpoint=True: i * step + start with step = (stop - start) / (num - 1), the last
// point set to `stop` itself
void np_linspace(double start, double stop, int num, std::vector<double>& y) {
    y.resize(num);
    const int div = num - 1;
    const double delta = stop - start;
    if (div > 0) {
        const double step = delta / div;
        for (int i = 0; i < num; ++i) y[i] = (step == 0.0 ? ((double)i / div) * delta : (double)i * step) + start;
        y[num - 1] = stop;
    } else {
        for (int i = 0; i < num; ++i) y[i] = (double)i * delta + start;
    }
}

void betas_of(int schedule_type, int timesteps, double max_beta, std::vector<double>& betas) {
    if (schedule_type == DSD_SCHEDULE_LINEAR) {
        np_linspace(1e-4, max_beta, timesteps, betas);
        return;
    }
    const int steps = timesteps + 1;
    const double s = 0.008, pi = 3.141592653589793;
    std::vector<double> x;
    np_linspace(0.0, (double)steps, steps, x);
    std::vector<double> ac(steps);
    for (int i = 0; i < steps; ++i) {
        const double c = cos(((x[i] / steps) + s) / (1 + s) * pi * 0.5);
        ac[i] = c * c;
    }
    const double ac0 = ac[0];
    for (int i = 0; i < steps; ++i) ac[i] = ac[i] / ac0;
    betas.resize(timesteps);
    for (int i = 0; i < timesteps; ++i) betas[i] = std::min(std::max(1 - (ac[i + 1] / ac[i]), 0.0), 0.999);
}

void tables_of(const std::vector<double>& betas, float* out) {
    const int n = (int)betas.size();
    double ac = 1.0;
    for (int i = 0; i < n; ++i) {
        const double b = betas[i], alpha = 1.0 - b, ac_prev = ac;         // cumprod; alphas_cumprod_prev[0] = 1
        ac = i == 0 ? alpha : ac * alpha;
        const double pv = b * (1.0 - ac_prev) / (1.0 - ac);
        const double row[DSD_DDPM_TABLES] = {b,
                                     ac,
                                     ac_prev,
                                     sqrt(ac),
                                     sqrt(1.0 - ac),
                                     log(1.0 - ac),
                                     sqrt(1.0 / ac),
                                     sqrt(1.0 / ac - 1),
                                     pv,
                                     log(std::max(pv, 1e-20)),
                                     b * sqrt(ac_prev) / (1.0 - ac),
                                     (1.0 - ac_prev) * sqrt(alpha) / (1.0 - ac)};
        for (int k = 0; k < DSD_DDPM_TABLES; ++k) out[(size_t)k * n + i] = (float)row[k];
    }
}

// ------------------------------------------------------------------------------------------
// fp32 pieces of torch that schedule.py leans on
// ------------------------------------------------------------------------------------------
// torch.linspace(start, end, steps) for fp32 on the CPU (RangeFactoriesKernel.cpp), the two-sided rule: step = (end - start)
// / (steps - 1); element i is start + step * i in the first half and end - step * (steps - 1 - i) in the second.  torch's
// kernels for AVX2 and AVX-512 hosts are built with FMA contraction, so each element is ONE fused operation there - and
// here, explicitly (schedule.py's t_array and time steps, and the goldens recorded from the reference, carry that rounding).
void torch_linspace(float start, float end, int steps, std::vector<float>& out) {
    out.resize(steps);
    if (steps == 1) {
        out[0] = start;
        return;
    }
    const float step = (end - start) / (float)(steps - 1);
    const int halfway = steps / 2;
    for (int i = 0; i < steps; ++i)
        out[i] = i < halfway ? fmaf(step, (float)i, start) : fmaf(-step, (float)(steps - i - 1), end);
}

// discrete VP noise schedule (schedule.VPSchedule)
struct VPSchedule {
    std::vector<float> log_alpha, t_array;
    int total_N = 0;
    VPSchedule(const float* betas, int n, bool clip) {
        log_alpha.resize(n);
        double acc = 0.0;                               // torch's CPU cumsum accumulates fp32 in double
        for (int i = 0; i < n; ++i) {
            acc += (double)logf(1.0f - betas[i]);
            log_alpha[i] = 0.5f * (float)acc;
        }
        if (clip && n > 0) {                            // numerical_clip_alpha, clipped_lambda = -5.1
            std::vector<float> lambs(n);
            for (int i = 0; i < n; ++i) {
                const float log_sigma = 0.5f * logf(1.0f - expf(2.0f * log_alpha[i]));
                lambs[n - 1 - i] = log_alpha[i] - log_sigma;        // flipped: ascending
            }
            const int idx = (int)(std::lower_bound(lambs.begin(), lambs.end(), -5.1f) - lambs.begin());
            if (idx > 0) log_alpha.resize(n - idx);
        }
        total_N = (int)log_alpha.size();
        std::vector<float> full;
        torch_linspace(0.0f, 1.0f, total_N + 1, full);
        t_array.assign(full.begin() + 1, full.end());
    }
    // interpolate_fn's neighbour choice and fp32 expression
    float log_mean_coeff(float t) const {
        const std::vector<float>&xp = t_array, &yp = log_alpha;
        const int k = total_N;
        const int idx = (int)(std::lower_bound(xp.begin(), xp.end(), t) - xp.begin());
        int i0, i1;
        if (idx == 0) i0 = 0, i1 = 1;
        else if (idx == k) i0 = k - 2, i1 = k - 1;
        else i0 = idx - 1, i1 = idx;
        const float x0 = xp[i0], x1 = xp[i1], y0 = yp[i0], y1 = yp[i1];
        const float num = (t - x0) * (y1 - y0);
        return y0 + num / (x1 - x0);
    }
    float alpha(float t) const { return expf(log_mean_coeff(t)); }
    float std_(float t) const { return sqrtf(1.0f - expf(2.0f * log_mean_coeff(t))); }
    float lam(float t) const {
        const float lm = log_mean_coeff(t);
        return lm - 0.5f * logf(1.0f - expf(2.0f * lm));
    }
    float model_time(float t) const { return (t - (float)(1. / total_N)) * (float)total_N; }
    void time_uniform_steps(int steps, std::vector<float>& ts) const {
        torch_linspace(1.0f, (float)(1. / total_N), steps + 1, ts);
    }
};

struct Tables {
    const float* p;
    int n;
    float at(int table, int i) const { return p[(size_t)table * n + i]; }
};

// ------------------------------------------------------------------------------------------
// the samplers (schedule.py, function by function)
// ------------------------------------------------------------------------------------------
constexpr int X = 0, TMP = 1;

void ddpm_ancestral(Builder& b, const Tables& tb, int t_max, int t_lo, int noise_index0, int& n_noise) {
    int k = noise_index0;
    for (int i = t_max - 1; i >= t_lo; --i) {
        const double sr = tb.at(TB_SQRT_RECIP_AC, i), srm1 = tb.at(TB_SQRT_RECIPM1_AC, i);
        const double c1 = tb.at(TB_POST_C1, i), c2 = tb.at(TB_POST_C2, i);
        const Lin x_recon = of(X, sr) - of(DSD_SRC_MODEL, srm1);
        Lin mean = x_recon * c1 + of(X, c2);
        b.begin(X, (float)i);
        if (i > 0) {
            const float sigma = expf(0.5f * tb.at(TB_POST_LOGVAR, i));
            mean = mean + of(noise_src(k), (double)sigma);
        }
        ++k;
        b.emit(X, mean);
    }
    n_noise = k;
}

void ddim(Builder& b, const Tables& tb, int t_max, int interval) {
    int last = -1;
    for (int i = 0; i < t_max; i += interval) last = i;
    for (int i = last; i >= 0; i -= interval) {
        const double a_t = tb.at(TB_AC, i), a_prev = tb.at(TB_AC, std::max(i - interval, 0));
        const double c_eps = sqrt((1 - a_prev) / a_prev) - sqrt((1 - a_t) / a_t);
        const Lin expr = (of(X, 1.0 / sqrt(a_t)) + of(DSD_SRC_MODEL, c_eps)) * sqrt(a_prev);
        b.begin(X, (float)i);
        b.emit(X, expr);
    }
}

void plms(Builder& b, const Tables& tb, int t_max, int interval) {
    const int hist0 = 2;            // ring of 4 eps buffers: 2..5
    auto x_pred = [&](const Lin& x, const Lin& n, int i) {
        const double a_t = tb.at(TB_AC, i), a_prev = tb.at(TB_AC, std::max(i - interval, 0));
        const double a_t_sq = sqrt(a_t), a_prev_sq = sqrt(a_prev);
        const double c_x = 1.0 / (a_t_sq * (a_t_sq + a_prev_sq));
        const double c_n = 1.0 / (a_t_sq * (sqrt((1 - a_prev) * a_t) + sqrt((1 - a_t) * a_prev)));
        return x + (x * c_x - n * c_n) * (a_prev - a_t);
    };
    auto mod4 = [](int v) { return ((v % 4) + 4) % 4; };
    int last = -1;
    for (int i = 0; i < t_max; i += interval) last = i;
    int n_hist = 0;
    for (int i = last; i >= 0; i -= interval) {
        const int slot = hist0 + mod4(n_hist);
        const int prev[3] = {hist0 + mod4(n_hist - 1), hist0 + mod4(n_hist - 2), hist0 + mod4(n_hist - 3)};
        const Lin eps = of(DSD_SRC_MODEL);
        if (n_hist == 0) {
            b.begin(X, (float)i);
            b.emit(slot, eps);
            b.emit(TMP, x_pred(of(X), eps, i));
            b.begin(TMP, (float)std::max(i - interval, 0));
            const Lin prime = (of(slot) + eps) / 2.0;
            b.emit(X, x_pred(of(X), prime, i));
        } else {
            Lin prime;
            if (n_hist == 1) prime = (eps * 3.0 - of(prev[0])) / 2.0;
            else if (n_hist == 2) prime = (eps * 23.0 - of(prev[0]) * 16.0 + of(prev[1]) * 5.0) / 12.0;
            else prime = (eps * 55.0 - of(prev[0]) * 59.0 + of(prev[1]) * 37.0 - of(prev[2]) * 9.0) / 24.0;
            b.begin(X, (float)i);
            b.emit(slot, eps);
            b.emit(X, x_pred(of(X), prime, i));
        }
        ++n_hist;
    }
}

// the fp32 scalars of the noise schedule at the solver's time steps
struct StepScalars {
    std::vector<float> ts, alpha, sigma, lam;
    StepScalars(const VPSchedule& ns, int steps) {
        ns.time_uniform_steps(steps, ts);
        for (float t : ts) {
            alpha.push_back(ns.alpha(t));
            sigma.push_back(ns.std_(t));
            lam.push_back(ns.lam(t));
        }
    }
};

void dpm_solver_pp(Builder& b, const float* betas, int n_betas, int steps, const char** why) {
    const VPSchedule ns(betas, n_betas, true);
    if (ns.total_N < 2) {
        *why = "fewer than 2 schedule points are left under the lambda clip";
        return;
    }
    const StepScalars s(ns, steps);
    const int XB = 0, slots[2] = {1, 2};
    auto data_pred = [&](int i, const Lin& x) { return (x - of(DSD_SRC_MODEL, s.sigma[i])) / (double)s.alpha[i]; };
    auto first_update = [&](const Lin& x, int i_s, int i_t, const Lin& m_s) {
        const float h = s.lam[i_t] - s.lam[i_s];
        const float sig = s.sigma[i_t] / s.sigma[i_s];
        const float coef = s.alpha[i_t] * expm1f(-h);
        return x * (double)sig - m_s * (double)coef;
    };
    auto second_update = [&](const Lin& x, int i1, int i0, int i_t, const Lin& m1, const Lin& m0) {
        const float lam1 = s.lam[i1], lam0 = s.lam[i0], lam_t = s.lam[i_t];
        const float h_0 = lam0 - lam1, h = lam_t - lam0;
        const float r0 = h_0 / h;
        const float phi_1 = expm1f(-h);
        const float a_phi = s.alpha[i_t] * phi_1;
        const float sig = s.sigma[i_t] / s.sigma[i0];
        const Lin d1_0 = (m0 - m1) * (double)(1.0f / r0);
        return x * (double)sig - m0 * (double)a_phi - d1_0 * (double)(0.5f * a_phi);
    };
    for (int i = 0; i < steps; ++i) {
        b.begin(XB, ns.model_time(s.ts[i]));
        const Lin x = of(XB);
        const Lin m_new = data_pred(i, x);
        const int step = i + 1;
        Lin nxt;
        if (i == 0) {
            nxt = first_update(x, 0, 1, m_new);
        } else {
            const int order = steps < 10 ? std::min(2, steps + 1 - step) : 2;       // lower_order_final
            if (order == 1) nxt = first_update(x, i, step, m_new);
            else nxt = second_update(x, i - 1, i, step, of(slots[(i - 1) % 2]), m_new);
        }
        if (i < steps - 1) b.emit(slots[i % 2], m_new);
        b.emit(XB, nxt);
    }
}

void unipc(Builder& b, const float* betas, int n_betas, int steps, const char** why) {
    const VPSchedule ns(betas, n_betas, false);
    if (ns.total_N < 2) {
        *why = "fewer than 2 schedule points";
        return;
    }
    const StepScalars s(ns, steps);
    const int XP = 0, XT = 1, slots[2] = {2, 3};
    struct Coeffs {
        double sig, a_hphi1, a_bh, rk, rho_first, rho_last;
    };
    // the scalar pieces of multistep_uni_pc_bh_update from ts[i0] to ts[i_t]
    auto coeffs = [&](int i0, int i_t, int order, int i1) {
        const float lam0 = s.lam[i0], lam_t = s.lam[i_t];
        const float h = lam_t - lam0;
        const float sig = s.sigma[i_t] / s.sigma[i0];
        const float alpha_t = s.alpha[i_t];
        const float rk = order == 2 ? (s.lam[i1] - lam0) / h : 1.0f;
        const float hh = -h;
        const float h_phi_1 = expm1f(hh);
        float h_phi_k = h_phi_1 / hh - 1.0f;
        const float b_h = expm1f(hh);
        float bvec[2] = {0.0f, 0.0f};
        int fact = 1;
        for (int i = 1; i <= order; ++i) {
            bvec[i - 1] = h_phi_k * (float)fact / b_h;
            fact *= (i + 1);
            h_phi_k = h_phi_k / hh - (float)(1.0 / fact);
        }
        Coeffs c;
        c.sig = sig;
        c.a_hphi1 = alpha_t * h_phi_1;
        c.a_bh = alpha_t * b_h;
        c.rk = rk;
        if (order == 1) {
            c.rho_first = c.rho_last = 0.5;
        } else {
            // torch.linalg.solve([[1, 1], [rk, 1]], bvec): LU with partial pivoting in fp32, as LAPACK's sgesv does it (the
            // multiplier is formed with the pivot's reciprocal)
            float a00 = 1.0f, a01 = 1.0f, a10 = rk, a11 = 1.0f, y0 = bvec[0], y1 = bvec[1];
            if (fabsf(a10) > fabsf(a00)) {
                std::swap(a00, a10);
                std::swap(a01, a11);
                std::swap(y0, y1);
            }
            const float l = a10 * (1.0f / a00);
            const float u11 = a11 - l * a01;
            y1 = y1 - l * y0;
            const float x1 = y1 / u11;
            const float x0 = (y0 - a01 * x1) / a00;
            c.rho_first = x0;
            c.rho_last = x1;
        }
        return c;
    };
    // eval 0: model at ts[0] on x_0 -> m_0; predictor to ts[1] (order 1: x_pred = x_t_)
    b.begin(XP, ns.model_time(s.ts[0]));
    const Lin m0 = (of(XP) - of(DSD_SRC_MODEL, s.sigma[0])) / (double)s.alpha[0];
    Coeffs c = coeffs(0, 1, 1, 0);
    Lin x_t_ = of(XP) * c.sig - m0 * c.a_hphi1;
    b.emit(slots[0], m0);
    b.emit(XT, x_t_);
    b.emit(XP, x_t_);
    Coeffs pc = c;
    int p_order = 1, p_m0_slot = slots[0], p_m1_slot = -1;
    for (int i = 1; i < steps; ++i) {
        // eval i: model at ts[i] on the predicted x (XP) -> m_t; corrector -> x_i; then predictor to ts[i + 1]
        b.begin(XP, ns.model_time(s.ts[i]));
        const Lin m_t = (of(XP) - of(DSD_SRC_MODEL, s.sigma[i])) / (double)s.alpha[i];
        const Lin m_prev0 = of(p_m0_slot);
        Lin corr;
        if (p_order == 2) {
            const Lin d1 = (of(p_m1_slot) - m_prev0) / pc.rk;
            corr = d1 * pc.rho_first;
        }
        const Lin x_i = of(XT) - (corr + (m_t - m_prev0) * pc.rho_last) * pc.a_bh;
        const int step = i + 1;
        const int order = std::min(2, steps + 1 - step);
        const bool use_corr = step != steps;
        c = coeffs(i, step, order, i - 1);
        x_t_ = x_i * c.sig - m_t * c.a_hphi1;
        Lin x_pred = x_t_;
        if (order == 2) {
            const Lin d1 = (m_prev0 - m_t) / c.rk;
            x_pred = x_t_ - d1 * (0.5 * c.a_bh);
        }
        const int new_slot = slots[i % 2];
        if (use_corr) {
            b.emit(new_slot, m_t);
            b.emit(XT, x_t_);
        }
        b.emit(XP, x_pred);
        pc = c;
        p_order = order;
        p_m0_slot = new_slot;
        p_m1_slot = slots[(i - 1) % 2];
    }
}

void reflow(Builder& b, int sampler, int steps, double t_start, double time_scale_factor) {
    const double dt = (1.0 - t_start) / std::max(1, steps);
    const float dts = (float)dt, tsf = (float)time_scale_factor;
    const int K1 = 2, K2 = 3, K3 = 4, K4 = 5, K5 = 6, M = DSD_SRC_MODEL;
    const Lin x = of(X), m = of(M);
    for (int i = 0; i < steps; ++i) {
        const float t = (float)t_start + (float)i * dts;
        // time_scale_factor * (t + off * dt) in the reference's fp32 order
        auto tt = [&](double off) { return off != 0.0 ? tsf * (t + (float)(off * dt)) : tsf * t; };
        if (sampler == DSD_SAMPLER_RF_EULER) {
            b.begin(X, tt(0)); b.emit(X, x + m * dt);
        } else if (sampler == DSD_SAMPLER_RF_RK2) {
            b.begin(X, tt(0)); b.emit(TMP, x + m * (0.5 * dt));
            b.begin(TMP, tt(0.5)); b.emit(X, x + m * dt);
        } else if (sampler == DSD_SAMPLER_RF_RK4) {
            b.begin(X, tt(0)); b.emit(K1, m); b.emit(TMP, x + m * (0.5 * dt));
            b.begin(TMP, tt(0.5)); b.emit(K2, m); b.emit(TMP, x + m * (0.5 * dt));
            b.begin(TMP, tt(0.5)); b.emit(K3, m); b.emit(TMP, x + m * dt);
            b.begin(TMP, tt(1.0));
            b.emit(X, x + (of(K1) + of(K2) * 2.0 + of(K3) * 2.0 + m) * (dt / 6.0));
        } else {
            const Lin k1 = of(K1), k2 = of(K2), k3 = of(K3), k4 = of(K4), k5 = of(K5);
            b.begin(X, tt(0)); b.emit(K1, m); b.emit(TMP, x + m * (0.25 * dt));
            b.begin(TMP, tt(0.25)); b.emit(K2, m); b.emit(TMP, x + (m + k1) * (0.125 * dt));
            b.begin(TMP, tt(0.25)); b.emit(K3, m); b.emit(TMP, x + (m * 2.0 - k2) * (0.5 * dt));
            b.begin(TMP, tt(0.5)); b.emit(K4, m); b.emit(TMP, x + (k1 * 3.0 + m * 9.0) * (0.0625 * dt));
            b.begin(TMP, tt(0.75)); b.emit(K5, m);
            b.emit(TMP, x + (k1 * -3.0 + k2 * 2.0 + k3 * 12.0 - k4 * 12.0 + m * 8.0) * (dt / 7.0));
            b.begin(TMP, tt(1.0));
            b.emit(X, x + (k1 * 7.0 + k3 * 32.0 + k4 * 12.0 + k5 * 32.0 + m * 7.0) * (dt / 90.0));
        }
    }
}

// RectifiedFlowONNX's euler loop: dt and the step times are fp32 tensor arithmetic there
void reflow_onnx(Builder& b, int steps, double t_start, double time_scale_factor) {
    const float ts = (float)t_start, tsf = (float)time_scale_factor;
    const float dt = (1.0f - ts) / (float)std::max(1, steps);
    const Lin x = of(X), m = of(DSD_SRC_MODEL);
    for (int i = 0; i < steps; ++i) {
        const float prod = (float)i * dt;
        const float time = prod + ts;
        b.begin(X, time * tsf);
        b.emit(X, x + m * (double)dt);
    }
}

bool is_ddpm_family(int s) { return s >= DSD_SAMPLER_DDPM && s <= DSD_SAMPLER_UNIPC; }
bool is_reflow(int s) { return s >= DSD_SAMPLER_RF_EULER && s <= DSD_SAMPLER_RF_EULER_ONNX; }

int tables_fill(const char* who, int32_t schedule_type, int32_t timesteps, double max_beta, float* out) {
    if (!out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (schedule_type != DSD_SCHEDULE_LINEAR && schedule_type != DSD_SCHEDULE_COSINE)
        return fail(nullptr, DSD_EINVAL, "%s: unknown schedule_type %d", who, schedule_type);
    if (timesteps < 1) return fail(nullptr, DSD_EINVAL, "%s: timesteps %d must be positive", who, timesteps);
    std::vector<double> betas;
    betas_of(schedule_type, timesteps, max_beta, betas);
    tables_of(betas, out);
    return DSD_OK;
}

int program_build(const char* who, const dsd_sampler_spec* spec, dsd_program** out) {
    if (!spec || !out) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (spec->struct_size != (int32_t)sizeof(dsd_sampler_spec))
        return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, spec->struct_size, sizeof(dsd_sampler_spec));
    const int s = spec->sampler;
    if (!is_ddpm_family(s) && !is_reflow(s)) return fail(nullptr, DSD_EINVAL, "%s: unknown sampler %d", who, s);

    Builder b;
    int n_bufs = 1, n_noise = 0;
    if (is_ddpm_family(s)) {
        const int t_max = spec->t_max, speedup = spec->speedup;
        if (spec->timesteps < 1) return fail(nullptr, DSD_EINVAL, "%s: timesteps %d must be positive", who, spec->timesteps);
        if (!spec->tables) return fail(nullptr, DSD_EINVAL, "%s: null tables", who);
        if (t_max < 0 || t_max > spec->timesteps)
            return fail(nullptr, DSD_EINVAL, "%s: t_max %d outside [0, timesteps = %d]", who, t_max, spec->timesteps);
        if (speedup < 1) return fail(nullptr, DSD_EINVAL, "%s: speedup %d must be at least 1", who, speedup);
        const Tables tb = {spec->tables, spec->timesteps};
        if (t_max == 0) {
            // the empty program: the loop of ddpm.py:244-349 over no step
        } else if (s == DSD_SAMPLER_DDPM) {
            if (spec->t_lo < 0 || spec->t_lo > t_max)
                return fail(nullptr, DSD_EINVAL, "%s: t_lo %d outside [0, t_max = %d]", who, spec->t_lo, t_max);
            if (spec->noise_index0 < 0 || spec->noise_index0 > INT32_MAX - 1000 - t_max)
                return fail(nullptr, DSD_EINVAL, "%s: noise_index0 %d out of range", who, spec->noise_index0);
            ddpm_ancestral(b, tb, t_max, spec->t_lo, spec->noise_index0, n_noise);
        } else if (s == DSD_SAMPLER_DDIM) {
            ddim(b, tb, t_max, speedup);
        } else if (s == DSD_SAMPLER_PLMS) {
            plms(b, tb, t_max, speedup);
            n_bufs = 6;
        } else {
            const int steps = t_max / speedup;
            if (steps < 2)
                return fail(nullptr, DSD_EINVAL, "%s: %s needs steps = t_max / speedup >= 2 (t_max %d, speedup %d)", who,
                            s == DSD_SAMPLER_UNIPC ? "UniPC" : "DPM-Solver++", t_max, speedup);
            const char* why = nullptr;
            if (s == DSD_SAMPLER_DPM_SOLVER_PP) {
                dpm_solver_pp(b, spec->tables, t_max, steps, &why);
                n_bufs = 3;
            } else {
                unipc(b, spec->tables, t_max, steps, &why);
                n_bufs = 4;
            }
            if (why) return fail(nullptr, DSD_EINVAL, "%s: %s", who, why);
        }
    } else {
        if (spec->steps < 0) return fail(nullptr, DSD_EINVAL, "%s: steps %d must not be negative", who, spec->steps);
        if (!(spec->t_start == spec->t_start) || !(spec->time_scale_factor == spec->time_scale_factor))
            return fail(nullptr, DSD_EINVAL, "%s: t_start or time_scale_factor is NaN", who);
        if (s == DSD_SAMPLER_RF_EULER_ONNX) reflow_onnx(b, spec->steps, spec->t_start, spec->time_scale_factor);
        else reflow(b, s, spec->steps, spec->t_start, spec->time_scale_factor);
        n_bufs = s == DSD_SAMPLER_RF_RK5 ? 7 : (s == DSD_SAMPLER_RF_RK4 ? 5 : 2);
    }
    if (b.err == 1) return fail(nullptr, DSD_EINVAL, "%s: a linear combination exceeds DSD_MAX_TERMS = %d", who, DSD_MAX_TERMS);
    if (b.err == 2) return fail(nullptr, DSD_EINVAL, "%s: an evaluation exceeds DSD_MAX_OUT = %d outputs", who, DSD_MAX_OUT);

    // one allocation: the dsd_program, then its evaluations
    const size_t n = b.evals.size();
    static_assert(sizeof(dsd_program) % alignof(dsd_eval) == 0, "the evaluations follow the program struct");
    char* mem = (char*)malloc(sizeof(dsd_program) + n * sizeof(dsd_eval));
    if (!mem) return fail(nullptr, DSD_ENOMEM, "%s: out of host memory for %zu evaluations", who, n);
    dsd_program* p = (dsd_program*)mem;
    dsd_eval* evals = (dsd_eval*)(mem + sizeof(dsd_program));
    if (n) memcpy(evals, b.evals.data(), n * sizeof(dsd_eval));
    p->n_bufs = n_bufs;
    p->result_buf = 0;
    p->n_evals = (int32_t)n;
    p->n_noise = n_noise;
    p->evals = n ? evals : nullptr;
    *out = p;
    return DSD_OK;
}

// nothing is thrown across the ABI: the builders' std::vectors are the only thing here that can throw
template <typename F>
int guarded(const char* who, F&& body) {
    try {
        return body();
    } catch (const std::exception&) {      // std::bad_alloc, or std::length_error from a vector
        return fail(nullptr, DSD_ENOMEM, "%s: out of host memory", who);
    }
}

}  // namespace

extern "C" {

int dsd_ddpm_tables_fill(int32_t schedule_type, int32_t timesteps, double max_beta, float* out) {
    const char* who = "dsd_ddpm_tables_fill";
    return guarded(who, [&] { return tables_fill(who, schedule_type, timesteps, max_beta, out); });
}

int dsd_program_build(const dsd_sampler_spec* spec, dsd_program** out) {
    const char* who = "dsd_program_build";
    return guarded(who, [&] { return program_build(who, spec, out); });
}

void dsd_program_free(dsd_program* prog) { free(prog); }

int dsd_onnx_ddpm_plan(int32_t timesteps, int32_t k_step, const int64_t* factors, int32_t n_factors, int32_t steps,
                       double depth, int32_t* t_max, int32_t* speedup) {
    const char* who = "dsd_onnx_ddpm_plan";
    if (!t_max || !speedup) return fail(nullptr, DSD_EINVAL, "%s: null argument", who);
    if (timesteps < 1 || k_step < 0 || steps < 1)
        return fail(nullptr, DSD_EINVAL, "%s: timesteps %d and steps %d must be positive, k_step %d not negative", who, timesteps,
                    steps, k_step);
    if (depth < 0) {            // no shallow source: the speed-up snaps DOWN to a factor of `timesteps`
        if (!factors || n_factors < 1) return fail(nullptr, DSD_EINVAL, "%s: no factors", who);
        const int64_t want = std::max(1, timesteps / steps);
        int count = 0;
        for (int i = 0; i < n_factors; ++i) count += factors[i] <= want;
        if (count == 0) return fail(nullptr, DSD_EINVAL, "%s: no factor is <= %d", who, (int)want);
        const int64_t f = factors[count - 1];
        if (f < 1 || f > INT32_MAX) return fail(nullptr, DSD_EINVAL, "%s: factor %lld out of range", who, (long long)f);
        *t_max = k_step;
        *speedup = (int32_t)f;
        return DSD_OK;
    }
    if (!(depth == depth)) return fail(nullptr, DSD_EINVAL, "%s: depth is NaN", who);
    const float scaled = (float)depth * (float)timesteps;
    const float rounded = nearbyintf(scaled);                   // torch.round: half to even (the default rounding mode)
    const int64_t d = rounded >= 9.0e18f ? INT64_MAX : (int64_t)rounded;
    const int64_t depth_i = std::min<int64_t>(d, k_step);
    const int64_t sp = std::max<int64_t>(1, depth_i / steps);
    *t_max = (int32_t)(depth_i / sp * sp);
    *speedup = (int32_t)sp;
    return DSD_OK;
}

}  // extern "C"
