// Radial profiles of the parametric sources (GaussianMorphology / SpergelMorphology, reference
// morphology.py:210-473) and their partial derivatives, in double.  Host and device code: the
// functions carry no state, so a CPU build can check them against scipy.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SMI_HD __host__ __device__
#else
#define SMI_HD
#endif

namespace smi {

enum { kProfileGaussian = 0, kProfileSpergel = 1 };
// layout of the six doubles of a profile component (parameters, moments, gradients)
enum { kPcy = 0, kPcx = 1, kPradius = 2, kPe1 = 3, kPe2 = 4, kPnu = 5, kProfileDoubles = 6 };

// 1 / Gamma(1 + mu), 1 / Gamma(1 - mu) and the two combinations Temme's series needs,
//     Gamma_1 = (1 / Gamma(1 - mu) - 1 / Gamma(1 + mu)) / (2 mu),   Gamma_2 = their mean,
// for |mu| <= 1/2 from the Taylor series 1 / Gamma(z) = sum_k c_k z^k (Abramowitz & Stegun
// 6.1.34): odd and even terms separate, so Gamma_1 has no cancellation at mu -> 0.
SMI_HD inline void temme_gammas(double mu, double &Gamma_1, double &Gamma_2,
                                double &inv_gamma_plus, double &inv_gamma_minus) {
    const double c[26] = {0.0,
                          1.0,
                          0.5772156649015329,
                          -0.6558780715202538,
                          -0.0420026350340952,
                          0.1665386113822915,
                          -0.0421977345555443,
                          -0.0096219715278770,
                          0.0072189432466630,
                          -0.0011651675918591,
                          -0.0002152416741149,
                          0.0001280502823882,
                          -0.0000201348547807,
                          -0.0000012504934821,
                          0.0000011330272320,
                          -0.0000002056338417,
                          0.0000000061160950,
                          0.0000000050020075,
                          -0.0000000011812746,
                          0.0000000001043427,
                          0.0000000000077823,
                          -0.0000000000036968,
                          0.0000000000005100,
                          -0.0000000000000206,
                          -0.0000000000000054,
                          0.0000000000000014};
    // 1 / Gamma(1 + mu) = sum_k c_k mu^(k - 1): even powers of mu from odd k, odd from even k
    const double m2 = mu * mu;
    double even = 0.0, odd = 0.0;  // Horner in mu^2
    for (int k = 25; k >= 1; k -= 2) even = even * m2 + c[k];
    for (int k = 24; k >= 2; k -= 2) odd = odd * m2 + c[k];
    Gamma_2 = even;
    Gamma_1 = -odd;
    inv_gamma_plus = even + mu * odd;
    inv_gamma_minus = even - mu * odd;
}

// K_a(x) and K_{a+1}(x) of the modified Bessel function of the second kind for a >= 0, x > 0.
// Both methods work at the fractional order mu = a - round(a), |mu| <= 1/2, and the upward
// recurrence K_{n+1} = (2 n / x) K_n + K_{n-1}, stable for K, carries the pair to the order a.
// Written from the papers, in their notation:
//   x < 2:  N. M. Temme, J. Comput. Phys. 19 (1975) 324:
//           K_mu = sum_k c_k f_k,  K_{mu+1} = (2 / x) sum_k c_k h_k,  c_k = (x^2 / 4)^k / k!,
//           f_k = (k f_{k-1} + p_{k-1} + q_{k-1}) / (k^2 - mu^2),  h_k = p_k - k f_k,
//           p_k = p_{k-1} / (k - mu),  q_k = q_{k-1} / (k + mu),
//           p_0 = Gamma(1 + mu) (2 / x)^mu / 2,  q_0 = Gamma(1 - mu) (x / 2)^mu / 2,
//           f_0 = (mu pi / sin mu pi) (Gamma_1 cosh sigma + Gamma_2 ln(2 / x) sinh sigma / sigma),
//           sigma = mu ln(2 / x).
//   x >= 2: the continued fraction of the same paper as arranged by I. J. Thompson and
//           A. R. Barnett, Comput. Phys. Commun. 47 (1987) 245 ("CF2"), summed forward with
//           Steed's algorithm: with a_1 = 1/4 - mu^2, a_{n+1} = a_n - 2 n (sign convention of the
//           recurrence below), b_n = 2 (n + x),
//           K_mu = sqrt(pi / 2 x) e^{-x} / S,  S = 1 + sum_n Q_n dh_n,  Q_n = sum_{k<=n} C_k q_k,
//           K_{mu+1} / K_mu = (mu + x + 1/2 - a_1 h) / x,  h = 1 / (b_1 + a_2 / (b_2 + ...)).
SMI_HD inline void bessel_k_pair(double a, double x, double &k_a, double &k_a1) {
    const double kEps = 1e-16, kPi = 3.141592653589793;
    const int order_steps = (int)(a + 0.5);
    const double mu = a - order_steps, mu2 = mu * mu;
    const double inv_x = 1.0 / x, two_over_x = 2.0 * inv_x;
    double k_lo, k_hi;  // K_mu, K_{mu+1}, then the pair moving up in the order
    if (x < 2.0) {
        const double half_x = 0.5 * x, pi_mu = kPi * mu;
        const double ln_2_over_x = -log(half_x), sigma = mu * ln_2_over_x;
        const double mu_pi_over_sin = fabs(pi_mu) < kEps ? 1.0 : pi_mu / sin(pi_mu);
        const double sinh_over_sigma = fabs(sigma) < kEps ? 1.0 : sinh(sigma) / sigma;
        double Gamma_1, Gamma_2, inv_gamma_plus, inv_gamma_minus;
        temme_gammas(mu, Gamma_1, Gamma_2, inv_gamma_plus, inv_gamma_minus);
        double f_k = mu_pi_over_sin *
                     (Gamma_1 * cosh(sigma) + Gamma_2 * sinh_over_sigma * ln_2_over_x);
        const double two_over_x_to_mu = exp(sigma);
        double p_k = 0.5 * two_over_x_to_mu / inv_gamma_plus;
        double q_k = 0.5 / (two_over_x_to_mu * inv_gamma_minus);
        double c_k = 1.0, sum_f = f_k, sum_h = p_k;  // k = 0: h_0 = p_0
        const double quarter_x2 = half_x * half_x;
        for (int k = 1; k < 500; ++k) {
            f_k = (k * f_k + p_k + q_k) / (k * k - mu2);
            c_k *= quarter_x2 / k;
            p_k /= k - mu;
            q_k /= k + mu;
            const double term = c_k * f_k;
            sum_f += term;
            sum_h += c_k * (p_k - k * f_k);
            if (fabs(term) < fabs(sum_f) * kEps) break;
        }
        k_lo = sum_f;
        k_hi = sum_h * two_over_x;
    } else {
        const double a_1 = 0.25 - mu2;
        double b_n = 2.0 * (1.0 + x);
        double D_n = 1.0 / b_n, h = D_n, dh_n = D_n;  // Steed: h_1 = dh_1 = D_1 = 1 / b_1
        double q_before = 0.0, q_n = 1.0;             // q_0, q_1 of the three-term recurrence
        double a_n = -a_1, C_n = a_1, Q_n = a_1;
        double S = 1.0 + Q_n * dh_n;
        for (int n = 2; n < 10000; ++n) {
            a_n -= 2 * (n - 1);
            C_n = -a_n * C_n / n;
            const double q_next = (q_before - b_n * q_n) / a_n;
            q_before = q_n;
            q_n = q_next;
            Q_n += C_n * q_next;
            b_n += 2.0;
            D_n = 1.0 / (b_n + a_n * D_n);
            dh_n = (b_n * D_n - 1.0) * dh_n;
            h += dh_n;
            const double term = Q_n * dh_n;
            S += term;
            if (fabs(term / S) < kEps) break;
        }
        k_lo = sqrt(kPi / (2.0 * x)) * exp(-x) / S;
        k_hi = k_lo * (mu + x + 0.5 - a_1 * h) * inv_x;
    }
    for (int n = 1; n <= order_steps; ++n) {
        const double k_next = (mu + n) * two_over_x * k_hi + k_lo;
        k_lo = k_hi;
        k_hi = k_next;
    }
    k_a = k_lo;
    k_a1 = k_hi;
}

// digamma for x > 0: recurrence up to x >= 10, then the asymptotic series
SMI_HD inline double digamma_pos(double x) {
    double r = 0.0;
    while (x < 10.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double i2 = 1.0 / (x * x);
    const double tail = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 -
                        i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))));
    return r + log(x) - 0.5 / x - tail;
}

// c_nu of Spergel (2010), the stored quartic fit (morphology.py:442-470), and d c_nu / d nu
SMI_HD inline double spergel_cnu(double nu) {
    return (((-0.00788962 * nu + 0.0735303) * nu - 0.27770785) * nu + 0.99483285) * nu +
           1.25227402;
}
SMI_HD inline double spergel_dcnu(double nu) {
    return ((4 * -0.00788962 * nu + 3 * 0.0735303) * nu + 2 * -0.27770785) * nu + 0.99483285;
}

// What depends on the parameters but not on the pixel.
struct ProfileConsts {
    double cy, cx, r, e1, e2, nu;
    double s;                            // 1 / sqrt(1 - |e|^2)
    double cnu, dcnu, inv_gamma, psi;    // Spergel: c_nu, c_nu', 1 / Gamma(nu + 1), digamma(nu + 1)
};

SMI_HD inline ProfileConsts profile_consts(const double *p, int kind) {
    ProfileConsts k;
    k.cy = p[kPcy], k.cx = p[kPcx], k.r = p[kPradius], k.e1 = p[kPe1], k.e2 = p[kPe2];
    k.nu = p[kPnu];
    k.s = 1.0 / sqrt(1.0 - (k.e1 * k.e1 + k.e2 * k.e2));
    k.cnu = k.dcnu = k.inv_gamma = k.psi = 0.0;
    if (kind == kProfileSpergel) {
        k.cnu = spergel_cnu(k.nu);
        k.dcnu = spergel_dcnu(k.nu);
        k.inv_gamma = 1.0 / tgamma(k.nu + 1.0);
        k.psi = digamma_pos(k.nu + 1.0);
    }
    return k;
}

// f(R2) and its derivatives w.r.t. R2 and (Spergel) nu at fixed R2.
//
// The nu-derivative follows the reference's FIT, not calculus: the reference registers kv with
// defvjp(kv, None, ...) (morphology.py:380-381), so autograd drops dK_nu/dnu and keeps the paths
// through (u/2)^nu, Gamma(nu + 1) and c_nu only.  That is what is evaluated here.
template <int KIND>
SMI_HD inline void profile_radial(const ProfileConsts &k, double R2, bool partials, double &f,
                                  double &df_dR2, double &df_dnu) {
    if (KIND == kProfileGaussian) {
        f = exp(-R2 / 2);
        df_dR2 = -0.5 * f;
        df_dnu = 0.0;
        return;
    }
    const double rho = sqrt(R2 + 1e-4), u = rho * k.cnu;
    const double a = fabs(k.nu);  // K_{-nu} = K_nu
    double ka, ka1;
    bessel_k_pair(a, u, ka, ka1);
    const double pref = pow(0.5 * u, k.nu) * k.inv_gamma;
    f = pref * ka;
    if (!partials) {
        df_dR2 = df_dnu = 0.0;
        return;
    }
    // K_{nu-1} + K_{nu+1} is even in nu; K_{a-1} = K_{a+1} - (2 a / u) K_a
    const double ksum = 2.0 * ka1 - (2.0 * a / u) * ka;
    const double df_du = (k.nu / u) * f - pref * 0.5 * ksum;
    df_dR2 = df_du * k.cnu / (2.0 * rho);
    df_dnu = f * (log(0.5 * u) - k.psi) + df_du * rho * k.dcnu;
}

// The morphology at pixel (Y, X) of the frame and, if `d` is given, its partials in the layout
// of the six doubles (d[kPnu] = 0 for a Gaussian).
template <int KIND>
SMI_HD inline double profile_at(const ProfileConsts &k, double Y, double X, double *d) {
    const double y = Y - k.cy, x = X - k.cx;
    const double Xp = ((1.0 - k.e1) * x - k.e2 * y) * k.s;
    const double Yp = (-k.e2 * x + (1.0 + k.e1) * y) * k.s;
    const double ir2 = 1.0 / (k.r * k.r);
    const double R2 = (Yp * Yp + Xp * Xp) * ir2;
    double f, fR, fnu;
    profile_radial<KIND>(k, R2, d != nullptr, f, fR, fnu);
    if (d) {
        const double s = k.s, s2 = s * s;
        // d R2 / d (x, y); the centre enters with the opposite sign
        const double dx = 2.0 * (Xp * s * (1.0 - k.e1) - Yp * s * k.e2) * ir2;
        const double dy = 2.0 * (-Xp * s * k.e2 + Yp * s * (1.0 + k.e1)) * ir2;
        d[kPcy] = -fR * dy;
        d[kPcx] = -fR * dx;
        d[kPradius] = fR * (-2.0 * R2 / k.r);
        // d s / d e_i = e_i s^3
        const double dXp1 = k.e1 * s2 * Xp - s * x, dYp1 = k.e1 * s2 * Yp + s * y;
        const double dXp2 = k.e2 * s2 * Xp - s * y, dYp2 = k.e2 * s2 * Yp - s * x;
        d[kPe1] = fR * 2.0 * (Xp * dXp1 + Yp * dYp1) * ir2;
        d[kPe2] = fR * 2.0 * (Xp * dXp2 + Yp * dYp2) * ir2;
        d[kPnu] = fnu;
    }
    return f;
}

}  // namespace smi
