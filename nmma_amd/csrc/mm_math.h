// mm_math.h -- the scalar fp64 arithmetic of the multi-messenger parameter conversion (kernel mm_convert), host and device:
// source-frame masses, the quasi-universal relations and the NR ejecta fits of nmma/core/conversion.py, one row at a time, in the
// reference's operation order (build with -ffp-contract=off).  numpy's semantics where they differ from libm's: np.maximum /
// np.minimum propagate NaN, np.sign(NaN) is NaN, `x ** 2` on an array is x * x, a scalar base `10 ** x` is pow(10, x).
#pragma once
#include "em_math.h"

namespace nmma {
namespace mm {

constexpr double kGeomMsunKm = 1.476625038050125;          // geom_msun_km: G Msun / c^2 in km
constexpr double kMsunCgs = 1.988409870698051e33, kCCgs = 2.99792458e10;

NM_HD double np_maximum(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
NM_HD double np_minimum(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }
NM_HD double np_sign(double v) { return (v != v) ? v : (v > 0 ? 1.0 : (v < 0 ? -1.0 : 0.0)); }
NM_HD bool is_finite(double v) { return v - v == 0.0; }
NM_HD double ten_to(double v) { return pow(10.0, v); }

// bilby's chirp_mass_and_mass_ratio_to_total_mass / total_mass_and_mass_ratio_to_component_masses
NM_HD void component_masses(int mass_mode, double a, double b, double& m1, double& m2) {
    if (mass_mode == NMMA_MM_COMPONENT_MASSES) { m1 = a; m2 = b; return; }
    const double total = a * pow(1 + b, 1.2) / pow(b, 0.6);
    m1 = total / (1 + b);
    m2 = m1 * b;
}

// ---- radii_from_qur (:239-270)
NM_HD double lambda_to_compactness(double lam) {
    const double loglam = log(lam);
    return 0.371 - 0.0391 * loglam + 0.001056 * loglam * loglam;
}
NM_HD double mass_and_compactness_to_radius(double mass, double comp) { return comp < 0.5 ? mass / comp * kGeomMsunKm : 0.0; }
// bilby: component_masses_to_chirp_mass, component_masses_to_symmetric_mass_ratio, lambda_1_lambda_2_to_lambda_tilde
NM_HD double qur_r16(double m1, double m2, double l1, double l2) {
    const double mc = pow(m1 * m2, 0.6) / pow(m1 + m2, 0.2);
    const double eta = np_minimum((m1 * m2) / ((m1 + m2) * (m1 + m2)), 0.25);
    const double lp = l1 + l2, lm = l1 - l2;
    const double lt = 8.0 / 13.0 * ((1 + 7 * eta - 31 * (eta * eta)) * lp + sqrt(1 - 4 * eta) * (1 + 9 * eta - 11 * (eta * eta)) * lm);
    return mc * pow(lt / 0.0042, 1.0 / 6.0) * kGeomMsunKm;
}

// ---- BNSEjectaFitting (:468-742)
NM_HD double dynamic_mass_fitting_KrFo(double m1, double m2, double c1, double c2) {
    const double a = -9.3335, b = 114.17, c = -337.56, n = 1.5465;
    double mdyn = m1 * (a / c1 + b * pow(m2 / m1, n) + c * c1);
    mdyn += m2 * (a / c2 + b * pow(m1 / m2, n) + c * c2);
    mdyn *= 1e-3;
    return np_maximum(0.0, mdyn);
}
NM_HD double log10_disk_mass_fitting(double total_mass, double mass_ratio, double mtov, double r16) {
    const double a0 = -1.725, delta_a = -2.337, b0 = -0.564, delta_b = -0.437, c = 0.958, d = 0.057, beta = 5.879, q_trans = 0.886;
    const double k = -3.606 * mtov / r16 + 2.38;
    const double threshold_mass = k * mtov;
    const double xi = 0.5 * tanh(beta * (mass_ratio - q_trans));
    const double a = a0 + delta_a * xi, b = b0 + delta_b * xi;
    const double l = a * (1 + b * tanh((c - total_mass / threshold_mass) / d));
    return np_maximum(-3.0, l);
}

// ---- NSBHEjectaFitting (:332-466)
NM_HD double chibh2risco(double chi) {
    const double z1 = 1.0 + pow(1.0 - chi * chi, 1.0 / 3) * (pow(1 + chi, 1.0 / 3) + pow(1 - chi, 1.0 / 3));
    const double z2 = sqrt(3.0 * (chi * chi) + z1 * z1);
    return 3.0 + z2 - np_sign(chi) * sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2));
}
NM_HD double baryon_mass_NS(double m, double comp) { return m * (1.0 + 0.6 * comp / (1.0 - 0.5 * comp)); }
NM_HD double nsbh_dynamic_mass_fitting(double m1, double m2, double c2, double risco, double baryon) {
    const double a1 = 7.11595154e-03, a2 = 1.43636803e-03, a4 = -2.76202990e-02, n1 = -8.63604211e-01, n2 = -1.68399507;
    const double q = m2 / m1;
    double mdyn = a1 * pow(q, n1) * (1.0 - 2.0 * c2) / c2;
    mdyn += -a2 * pow(q, n2) * risco + a4;
    mdyn *= baryon;
    return np_maximum(0.0, mdyn);
}
NM_HD double remnant_disk_mass_fitting(double m1, double m2, double c2, double risco, double baryon) {
    const double a = 0.40642158, b = 0.13885773, c = 0.25512517, d = 0.761250847;
    const double q = m2 / m1;
    const double eta = q / ((1.0 + q) * (1.0 + q));
    double rem = a * pow(eta, -1.0 / 3.0) * (1.0 - 2.0 * c2);
    rem += -b * risco / eta * c2 + c;
    rem = np_maximum(rem, 0.0);
    rem = pow(rem, 1.0 + d);
    rem *= baryon;
    return rem;
}

// what the fits read of a row
struct FitInput {
    double m1, m2, r1, r2, mtov, r16, alpha, zeta, chi;
};

// bns_ejecta_conversion (:660-697): the three masses before the isfinite filter, and the disk mass for the jet energy
NM_HD void bns_ejecta(const FitInput& p, double out[3], double& log10_mdisk) {
    const double total_mass = p.m1 + p.m2, mass_ratio = p.m2 / p.m1;
    const double c1 = p.m1 * kGeomMsunKm / p.r1, c2 = p.m2 * kGeomMsunKm / p.r2;
    const double mdyn = dynamic_mass_fitting_KrFo(p.m1, p.m2, c1, c2);
    log10_mdisk = log10_disk_mass_fitting(total_mass, mass_ratio, p.mtov, p.r16 / kGeomMsunKm);
    out[0] = log10(mdyn + p.alpha);
    out[1] = log10(p.zeta) + log10_mdisk;
    out[2] = log10(ten_to(out[0]) + ten_to(out[1]));
}

// nsbh_parameter_conversion (:421-463)
NM_HD void nsbh_ejecta(const FitInput& p, double out[4]) {
    const double c2 = p.m2 * kGeomMsunKm / p.r2;
    const double risco = chibh2risco(p.chi), baryon = baryon_mass_NS(p.m2, c2);
    const double mdyn = nsbh_dynamic_mass_fitting(p.m1, p.m2, c2, risco, baryon);
    const double mdisk = remnant_disk_mass_fitting(p.m1, p.m2, c2, risco, baryon) - mdyn;
    const double mej_dyn = mdyn + p.alpha;
    out[0] = out[1] = -dinf();
    if (mdisk > 0.) {
        out[0] = log10(mej_dyn);
        out[1] = log10(mdisk) + log10(p.zeta);
    }
    out[2] = log10(ten_to(out[0]) + ten_to(out[1]));
    out[3] = -dinf();
}

// grb_energy_conversion (:699-709): log10 of the jet energy, and the top-hat jet's isotropic equivalent
NM_HD double log10_jet_energy(double eps, double zeta, double log10_mdisk, double log10_msun_erg) {
    double e = log10(eps);
    e += log10(1.0 - zeta);
    e += log10_mdisk + log10_msun_erg;
    return e;
}
NM_HD double tophat_log10_e0(double log10_ejet, double theta_core) {
    const double s = sin(theta_core / 2);
    return log10_ejet - log10(s * s);
}

// ---- the power-law jet's integral (:298-316): np.linspace(0, stop, 100) and scipy.integrate.simpson(x=x, y=y) for an EVEN number
// of samples (scipy/integrate/_quadrature.py): 49 three-node panels in the form for unequal spacings, whose divisions answer 0
// where the divisor is 0, then Cartwright's correction for the last interval.
constexpr int kJetNodes = 100, kJetPanels = 49;
NM_HD double jet_node_x(int i, double stop) { return i == kJetNodes - 1 ? stop : i * (stop / (kJetNodes - 1)); }
NM_HD double jet_node_y(double x, double theta_core, double b) {
    const double r = x / theta_core;
    return sin(x) * pow(1 + 1 / b * (r * r), -b / 2);
}
NM_HD double div0(double num, double den) { return den != 0 ? num / den : 0.0; }
template <class YPtr>
NM_HD double simpson_panel(int k, double stop, YPtr y) {
    const double x0 = jet_node_x(2 * k, stop), x1 = jet_node_x(2 * k + 1, stop), x2 = jet_node_x(2 * k + 2, stop);
    const double h0 = x1 - x0, h1 = x2 - x1;
    const double hsum = h0 + h1, hprod = h0 * h1, h0divh1 = div0(h0, h1);
    return hsum / 6.0 * (y[2 * k] * (2.0 - div0(1.0, h0divh1)) + y[2 * k + 1] * (hsum * div0(hsum, hprod)) + y[2 * k + 2] * (2.0 - h0divh1));
}
template <class YPtr>
NM_HD double simpson_last_interval(double stop, YPtr y) {
    const int n = kJetNodes;
    const double h0 = jet_node_x(n - 2, stop) - jet_node_x(n - 3, stop), h1 = jet_node_x(n - 1, stop) - jet_node_x(n - 2, stop);
    const double alpha = div0(2 * (h1 * h1) + 3 * h0 * h1, 6 * (h1 + h0));
    const double beta = div0(h1 * h1 + 3.0 * h0 * h1, 6 * h0);
    const double eta = div0(1 * (h1 * h1 * h1), 6 * h0 * (h0 + h1));
    return alpha * y[n - 1] + beta * y[n - 2] - eta * y[n - 3];
}
NM_HD double powerlaw_log10_e0(double log10_ejet, double integral) {
    const double eps_c = ten_to(log10_ejet) / (2 * kPi * integral);
    return log10(4 * kPi * eps_c);
}

}  // namespace mm
}  // namespace nmma
