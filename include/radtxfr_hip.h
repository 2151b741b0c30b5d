/*
 * radtxfr_hip.h -- C ABI of libradtxfr_hip.so, the MI355X (gfx950) engine behind the
 * reference's Python hot-path functions.
 *
 * The reference (westi024/RadTxfr) is 100 % Python and has no FFI of its own; its boundary for
 * this path is the set of Python call signatures listed in SURVEY.md section 8b. Each entry point
 * below is what a binding for one of those functions calls; the cited lines are the reference
 * code the entry point replaces. radtxfr_amd/_lib.py is the ctypes binding; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; rtx_last_error() gives the text
 *     (thread-local). No C++ exception crosses the ABI.
 *   - pointers are DEVICE pointers unless the name ends in _h (host).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). Calls are asynchronous
 *     with respect to the host and never allocate, free or synchronise, except the
 *     rtx_lines_* / rtx_prep_* create/free calls, which say so.
 *   - spectra are float32, wavenumber-contiguous; a layer-resolved array is layer-major
 *     ([n_layers][ld], element (k,i) at k*ld+i) so loads along the wavenumber axis coalesce.
 *   - the spectral grid is never materialised: X[i] = xmin + (offset+i)*step in fp64 (product
 *     then sum, unfused, as np.linspace builds it) and X[n_total-1] = xmax exactly.
 */
#ifndef RADTXFR_HIP_H
#define RADTXFR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_VERSION 100 /* major*10000 + minor*100 + patch */

/* Uniform spectral axis = np.linspace(xmin, xmax, n_total) as built by
 * radiative_transfer.py:251-271 (make_spectral_axis); [offset, offset+n) is the part this
 * call (this GPU) owns, so a wavenumber shard evaluates bit-identical grid values. */
typedef struct rtx_grid {
  double xmin;
  double xmax;
  double step; /* (xmax-xmin)/(n_total-1), the value np.linspace computes */
  int64_t n_total;
  int64_t offset;
  int64_t n;
} rtx_grid;

int rtx_version(void);
const char* rtx_last_error(void);
/* name[0..len) <- device name, *n_cu <- compute units, of the current HIP device */
int rtx_device_info(char* name_h, int len, int* n_cu_h);

/* ------------------------------------------------------------------------------------------
 * Line table. Replaces LOCAL_TABLE_CACHE[name]['data'] (misc/hapi.py:438-463) for the columns
 * absorptionCoefficient_Voigt reads (misc/hapi.py:11059-11125). Rows must be sorted by nu.
 * `species_h[l]` in [0,n_species) indexes the caller's list of distinct (molec_id,local_iso_id)
 * pairs; the per-species quantities of rtx_line_prep are given in that order.
 * n_self_h / deltap_air_h / delta_self_h may be NULL (hapi's fallbacks apply: n_self->n_air,
 * others 0; misc/hapi.py:11097-11125). Allocates device memory and synchronises. */
typedef struct rtx_lines rtx_lines;
int rtx_lines_create(int64_t n_lines, int n_species, const double* nu_h, const double* sw_h,
                     const double* elower_h, const double* gamma_air_h, const double* gamma_self_h,
                     const double* n_air_h, const double* n_self_h, const double* delta_air_h,
                     const double* deltap_air_h, const double* delta_self_h,
                     const int32_t* species_h, rtx_lines** out);
int rtx_lines_free(rtx_lines* lines);
int64_t rtx_lines_count(const rtx_lines* lines);
/* Optional speed-dependence columns SD_air / SD_self (misc/hapi.py:10884-10887), in the order of the rows given to
 * rtx_lines_create; either may be NULL (= 0). Only rtx_line_prep_profile(RTX_PROFILE_SDVOIGT) reads them. */
int rtx_lines_set_sd(rtx_lines* lines, const double* sd_air_h, const double* sd_self_h);
/* Optional deltap_self column: temperature dependence of the self-induced pressure shift,
 * Shift0 += abun_self * (delta_self + deltap_self*(T - Tref)) * p (misc/hapi.py:11120-11128). NULL = 0. */
int rtx_lines_set_deltap_self(rtx_lines* lines, const double* deltap_self_h);
/* Extra broadener column sets: the gamma_<sp>, n_<sp>, delta_<sp>, deltap_<sp> and SD_<sp> columns the reference reads for
 * any Diluent key other than air and self (misc/hapi.py:11090-11128; SD :10860-10890). Set j (0 <= j < n_extra) is column
 * set 2 + j of rtx_line_prep_mix (0 = air, 1 = self keep the columns of rtx_lines_create / _set_sd / _set_deltap_self).
 * Each argument is an array of n_extra host pointers, entry j the column of set j in the row order given to
 * rtx_lines_create (n_lines doubles), or NULL; a whole argument may be NULL. The reference's fallbacks: an absent gamma,
 * delta, deltap or SD column is 0, an absent n column is n_air (:11103-11110; a foreign n of 0 stays 0 -- only self falls
 * back where its n is 0). Replaces the previous set; n_extra = 0 drops it. Allocates device memory and synchronises. */
#define RTX_MAX_BROADENERS 64
int rtx_lines_set_broadeners(rtx_lines* lines, int n_extra, const double* const* gamma_h, const double* const* n_h,
                             const double* const* delta_h, const double* const* deltap_h, const double* const* sd_h);

/* ------------------------------------------------------------------------------------------
 * Per-(line, layer) prologue, fp64. Replaces the per-line environment block of
 * absorptionCoefficient_Voigt, misc/hapi.py:11068-11134: S(T) (:10169-10175), GammaD (:11085-
 * 11087), Gamma0 (:10183-10184), Shift0 (:11127-11128), OmegaWingF (:11131) and the two
 * bisect() window bounds (:11133-11134), for every line and every layer at once.
 *
 * Host inputs (small, copied with hipMemcpyAsync on `stream`; kept alive by the prep object):
 *   T_h[n_layers] K, p_atm_h[n_layers] atm
 *   qratio_h[n_species*n_layers]   Q(Tref)/Q(T_k) per species (TIPS, misc/hapi.py:11069-11070)
 *   weight_h[n_species*n_layers]   factor multiplying S(T) for that species in that layer:
 *       hapi path : factor/natural_abundance*abundance  (misc/hapi.py:11136-11137)
 *       OD path   : volumeConcentration(p,T)*x_m*PL*1e5  (SURVEY 8(a-3)); 0 drops the species
 *   mass_h[n_species]  g/mol (misc/hapi.py:11086)
 *   dil_air, dil_self  Diluent fractions (misc/hapi.py:11025-11032)
 *   omega_wing, omega_wing_hw  (misc/hapi.py:11131); intensity_threshold (:11082)
 *   scale  power of two folded into the fp32 strengths (HITRAN-unit cross sections are ~1e-25)
 * rtx_prep_create allocates (n_lines*max_layers records, plus per-tile line ranges for grids of up
 * to max_points points) and may synchronise; rtx_line_prep only enqueues work. One prep object
 * can be re-used for any atmospheric state / grid within its capacity. */
typedef struct rtx_prep rtx_prep;
int rtx_prep_create(const rtx_lines* lines, int max_layers, int64_t max_points, rtx_prep** out);
int rtx_prep_free(rtx_prep* prep);
int rtx_line_prep(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers,
                  const double* T_h, const double* p_atm_h, const double* qratio_h,
                  const double* weight_h, const double* mass_h, double dil_air, double dil_self,
                  double omega_wing, double omega_wing_hw, double intensity_threshold,
                  double scale, void* stream);
/* The same prologue for the other hapi profiles that share it; rtx_voigt_sum then sums whatever
 * profile the records describe. rtx_line_prep == profile RTX_PROFILE_VOIGT.
 *   RTX_PROFILE_LORENTZ  absorptionCoefficient_Lorentz, misc/hapi.py:11144-11375: PROFILE_LORENTZ (:10150),
 *                        OmegaWingF = max(OmegaWing, OmegaWingHW*Gamma0) (:11364)
 *   RTX_PROFILE_DOPPLER  absorptionCoefficient_Doppler, misc/hapi.py:11384-11559: PROFILE_DOPPLER (:10160), its own
 *                        GammaD constants (:11534-11538), OmegaWingF = max(OmegaWing, OmegaWingHW*GammaD) (:11540),
 *                        Shift0 = dil_air * delta_air * p (:11543; pass dil_air = 0 for LineShift=False) */
#define RTX_PROFILE_VOIGT 0
#define RTX_PROFILE_LORENTZ 1
#define RTX_PROFILE_DOPPLER 2
#define RTX_PROFILE_SDVOIGT 3 /* records for rtx_sdvoigt_sum (below); windows as for Voigt */
/* Hot tiles (line lists cluster: a band head puts thousands of candidate lines on one line-sum tile, and one workgroup per
 * tile would serialise the launch). The prologue bounds, on the host, the candidates any tile of `grid` can have -- no
 * window is wider than max(OmegaWing, OmegaWingHW * gamma, misc/hapi.py:11131) with the table's column extremes -- and
 * rtx_voigt_sum cuts tiles with more than 768 candidates into parts of 256 evaluated by extra workgroups and summed in a fixed
 * order (results stay bit-reproducible and independent of wavenumber sharding). This returns the number of extra parts
 * the last prologue allowed for: 0 = no tile of that table / grid can be hot and the extra kernels are never launched.
 * A bound that grows (new table or grid, much wider wings) re-allocates the part workspace inside rtx_line_prep*: the one
 * case in which a prologue call allocates and synchronises. */
int64_t rtx_prep_split_bound(const rtx_prep* prep);
int rtx_line_prep_profile(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers,
                          const double* T_h, const double* p_atm_h, const double* qratio_h,
                          const double* weight_h, const double* mass_h, double dil_air,
                          double dil_self, double omega_wing, double omega_wing_hw,
                          double intensity_threshold, double scale, int profile, void* stream);

/* The grid prologue with every line's window held at another temperature: T_win_h[n_layers] (host) replaces T_h in
 * OmegaWingF (misc/hapi.py:11131), hence in the windows bisect(X, nu -+ W) (:11133-11134), the candidate half-widths and
 * the hot-tile bound; strengths, partition sums, widths and shifts are taken at T_h as in rtx_line_prep_profile. With
 * T_win_h = T_h the records are those of rtx_line_prep_profile. Used for dOD/dT by central differences at T_h = T -+ h with
 * T_win_h = T: the derivative of the truncated line-sum with each line's support fixed (no cut-off steps). T_win_h is
 * copied into a device buffer owned by the prep object (grow-only: the first call allocates, hence synchronises).
 * profile RTX_PROFILE_VOIGT / _LORENTZ / _DOPPLER. Follow with rtx_voigt_sum. */
int rtx_line_prep_window(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers,
                         const double* T_h, const double* T_win_h, const double* p_atm_h, const double* qratio_h,
                         const double* weight_h, const double* mass_h, double dil_air, double dil_self,
                         double omega_wing, double omega_wing_hw, double intensity_threshold, double scale,
                         int profile, void* stream);

/* The prologue on an explicit axis X_h[nx] instead of a uniform grid (the reference sorts whatever OmegaGrid it is given
 * and bisects it, misc/hapi.py:10979-10983, 11133-11134): host fp64, non-decreasing, finite; 0 <= nx <= the max_points of
 * rtx_prep_create. X_h is copied into a device buffer owned by the prep object (grow-only: a longer axis than before
 * allocates, hence synchronises), so the caller may free it on return. Same per-line physics as rtx_line_prep_profile;
 * windows are bisect_right(X, nu -+ W) on the axis itself. profile RTX_PROFILE_VOIGT / _LORENTZ / _DOPPLER;
 * RTX_PROFILE_SDVOIGT is refused. No tile of an axis is ever cut (rtx_prep_split_bound does not apply). */
int rtx_line_prep_axis(rtx_prep* prep, const rtx_lines* lines, const double* X_h, int64_t nx, int n_layers,
                       const double* T_h, const double* p_atm_h, const double* qratio_h, const double* weight_h,
                       const double* mass_h, double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                       double intensity_threshold, double scale, int profile, void* stream);

/* The prologue with per-layer diluent mixes: Diluent of misc/hapi.py:11025-11032 as fractions per (diluent, species,
 * layer) over any column sets instead of two call-wide scalars. Arguments as rtx_line_prep_profile / rtx_line_prep_axis with
 * dil_air, dil_self replaced by
 *   n_dil              0 <= n_dil <= RTX_MAX_DILUENTS diluents
 *   dil_h[n_dil]       column set of each: 0 air, 1 self, 2 + j extra set j of rtx_lines_set_broadeners
 *   frac_h[n_dil][n_species][n_layers]   fractions (host; not validated, as the reference's range check never fires)
 * Per (line, layer), summed over the diluents in the caller's order (misc/hapi.py:11090-11128, 10884-10890):
 *   Gamma0 += f * gamma * p * (Tref/T)^n,  Shift0 += f * (delta + deltap * (T - Tref)) * p,
 *   Gamma2 += f * SD * p * gamma  (RTX_PROFILE_SDVOIGT; the un-scaled gamma column of each set).
 * A diluent may repeat (the reference sums keys that differ only in case: "AIR" and "air" are two entries of set 0). A zero
 * fraction contributes nothing. S(T), GammaD, windows, records and the hot-tile bound (which takes the largest
 * sum_d |f_d| gamma_max_d over species and layers with each set's n range) are those of the scalar prologues; with
 * {air: dil_air, self: dil_self} the records are theirs bit for bit. The fractions are copied into a device buffer owned by
 * the prep object (grow-only: the first call allocates, hence synchronises).
 * rtx_line_prep_mix: profile RTX_PROFILE_VOIGT / _LORENTZ / _SDVOIGT (Doppler takes no diluent, misc/hapi.py:11510-11513);
 * follow with rtx_voigt_sum, or rtx_sdvoigt_sum for SDVOIGT. rtx_line_prep_axis_mix: RTX_PROFILE_VOIGT / _LORENTZ; follow
 * with rtx_voigt_sum_axis. */
#define RTX_MAX_DILUENTS 8
int rtx_line_prep_mix(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers, const double* T_h,
                      const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                      int n_dil, const int32_t* dil_h, const double* frac_h, double omega_wing, double omega_wing_hw,
                      double intensity_threshold, double scale, int profile, void* stream);
int rtx_line_prep_axis_mix(rtx_prep* prep, const rtx_lines* lines, const double* X_h, int64_t nx, int n_layers,
                           const double* T_h, const double* p_atm_h, const double* qratio_h, const double* weight_h,
                           const double* mass_h, int n_dil, const int32_t* dil_h, const double* frac_h, double omega_wing,
                           double omega_wing_hw, double intensity_threshold, double scale, int profile, void* stream);

/* ------------------------------------------------------------------------------------------
 * Voigt line-sum. Replaces the per-line PROFILE_VOIGT + scatter-add loop, misc/hapi.py:11050,
 * 11135-11138 (PROFILE_VOIGT :10131 -> pcqsdhc PART1 :9900-9915 -> hum1_wei :9833-9844) with a
 * gather over the lines whose window covers each grid point.
 *   out_f32[n_layers][ld]  (may be NULL)   sum * 1            -> layer optical depths / k(nu)
 *   out_f64[n_layers][ld]  (may be NULL)   (double)sum/scale  -> hapi Xsect
 * compute_OD contract: radiative_transfer.py:395-456. */
/* points per line-sum workgroup tile (capacity granularity of rtx_prep_create) */
int rtx_voigt_tile_points(void);
int rtx_voigt_sum(const rtx_prep* prep, const rtx_grid* grid, int n_layers, float* out_f32,
                  double* out_f64, int64_t ld, void* stream);
/* rtx_voigt_sum's fp32 sum for a part of the column: layers [k_lo, k_hi) (an empty range enqueues nothing), and of those
 * layers only the rows nobody has said to skip. A row is 64 consecutive points counted from the shard's first, 16 rows make
 * a line-sum tile (rtx_voigt_tile_points()).
 *   skip_rows  device, one byte per row, padded to whole tiles (16 bytes per tile, ceil(n / tile points) tiles), 16-byte
 *              aligned, read by the kernels on `stream`; NULL: nothing is skipped. A row whose byte is not 0 is neither
 *              summed nor written: out_f32 keeps what it held there. A tile whose 16 rows are skipped loads no line record.
 * Every value written is rtx_voigt_sum's, bit for bit; layers outside [k_lo, k_hi) are not touched. This is the launch that
 * rtx_compute_tud_opts(RTX_CTUD_OD_SCRATCH) makes for its middle layers, with the caller's rows in place of the TUD pass's.
 * flags must be 0. Refused, with a message: the last prologue was an axis one; the table has a hot-tile bound
 * (rtx_prep_split_bound(prep) > 0: the parts kernels take no subset); RADTXFR_VOIGT_KERNEL=scatter (the point-by-point kernel
 * takes none either); a layer range outside [0, n_layers); skip_rows misaligned, or given for a table without lines. */
int rtx_voigt_sum_rows(const rtx_prep* prep, const rtx_grid* grid, int n_layers, float* out_f32, int64_t ld, int k_lo,
                       int k_hi, const unsigned char* skip_rows, void* stream, unsigned flags);
/* The line-sum on the axis of the last rtx_line_prep_axis (an error if the last prologue was a grid one, and
 * rtx_voigt_sum after an axis prologue is one too): out_*[n_layers][ld], ld >= nx, as for rtx_voigt_sum. Point by point
 * (no Chebyshev-node far wings), deterministic: repeated calls give identical bits. */
int rtx_voigt_sum_axis(const rtx_prep* prep, int n_layers, float* out_f32, double* out_f64, int64_t ld, void* stream);

/* Analytic temperature derivative of the Voigt line-sum (uniform grid, Voigt profile, call-wide dil_air / dil_self).
 * rtx_line_prep_dt: rtx_line_prep_profile's arguments without `profile`, plus
 *   dlnsw_h[n_species][n_layers]  (host) d ln(qratio * weight) / dT per species and layer, the two host inputs' own
 *                                 temperature dependence (for the optical-depth weights: -Q'(T)/Q(T) - 1/T).
 * It writes the records of rtx_line_prep_profile(..., RTX_PROFILE_VOIGT) bit for bit (rtx_voigt_sum may follow it) and,
 * in buffers owned by the prep object (grow-only: the first call allocates, hence synchronises), one derivative record
 * per (line, layer), formed in fp64.
 * rtx_voigt_sum_dt: out_*[n_layers][ld] as rtx_voigt_sum's, the sum over lines of d/dT [A K(x, y)] at the layer's
 * (T, p) with every line's window [lo, hi) held fixed: each point differentiates the branch of hum1_wei it is on
 * (misc/hapi.py:9833-9844), the step of that function at |x| + y = 15 is not differentiated. An error unless the last
 * prologue on `prep` was rtx_line_prep_dt. Point by point, deterministic: repeated calls give identical bits, and a shard
 * that starts on a multiple of rtx_voigt_tile_points() gives the bits of the full grid. Exact 0 outside every window. */
int rtx_line_prep_dt(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers, const double* T_h,
                     const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h,
                     const double* dlnsw_h, double dil_air, double dil_self, double omega_wing, double omega_wing_hw,
                     double intensity_threshold, double scale, void* stream);
int rtx_voigt_sum_dt(const rtx_prep* prep, const rtx_grid* grid, int n_layers, float* out_f32, double* out_f64,
                     int64_t ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * Planck radiance. Replaces planckian(), radiative_transfer.py:792-848.
 *   X == NULL : spectral axis = grid; else X[nx] (fp64 wavenumbers or micrometres)
 *   out[nx][nT] float64 (C order, spectral axis first, as the reference returns it) */
int rtx_planck(const rtx_grid* grid, const double* X, int64_t nx, const double* T, int64_t nT,
               int wavelength, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Brightness temperature and its inverse. Replace brightnessTemperature(),
 * radiative_transfer.py:851-933, and BT2L(), :936-1014 (fp64; bad_value where the reference masks:
 * non-finite or non-positive radiance :922-923, non-finite radiance or T<=0 :1004-1005).
 *   X[nx] fp64; in/out [nx][m] fp64, spectral axis first. */
int rtx_brightness_temperature(const double* X, int64_t nx, const double* L, int64_t m,
                               int wavelength, double bad_value, double* T_out, void* stream);
int rtx_bt2l(const double* X, int64_t nx, const double* T, int64_t m, int wavelength,
             double bad_value, double* L_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * TUD integration. Replaces the body of compute_TUD after the OD loop,
 * radiative_transfer.py:340-392: on-the-fly Planck, tau, upwelling recurrence (:346-356),
 * N_angle-stream downwelling recurrence and its cos*sin average (:368-389).
 *   OD[n_layers][ld] float32;  T_h[n_layers];
 *   n_alt sensor altitudes: mask_h[a*n_layers+k] = (Z[k] <= zs[a]) (:348), count = popcount;
 *   n_mu slant factors mu_h (:313);  n_down = layers the downwelling loop covers (quirk: the
 *   count of the LAST altitude, :353,370);
 *   outputs: tau[n_alt*n_mu][ld_out], Lu[n_alt*n_mu][ld_out] (index a*n_mu+m), Ld[ld_out];
 *   Ld_angles: NULL, or [n_angle][ld_out] per-stream downwelling radiances (what opts['save']
 *   dumps as Ld, :374-386);
 *   return_od != 0 puts sum(OD*mu) in the tau slot (:349-350).
 * The weighted stream sum is evaluated as sum_k B_k [G(S_k) - G(S_k+1)], G(S) = sum_q w_q exp(-S/cos
 * theta_q) tabulated per n_angle in fp64 (the same quadrature, summed over the angles first); with
 * Ld_angles the streams themselves are run (both against the reference's recurrence to <= 1e-5). */
int rtx_tud(const float* OD, int64_t ld, const rtx_grid* grid, int n_layers, const double* T_h,
            int n_alt, const uint8_t* mask_h, int n_mu, const double* mu_h, int n_down,
            int n_angle, int return_od, float* tau, float* Lu, float* Ld, float* Ld_angles,
            int64_t ld_out, void* stream);
/* rtx_tud with promises about its input. flags = 0 is rtx_tud. RTX_TUD_OD_NONNEG: the caller vouches that every OD value is
 * finite and >= 0. One (altitude, slant) pair with return_od == 0 and a mask that is its first count layers, on a grid fine
 * enough for the Planck-node kernel (63 steps x (4/nu_min + c2/T_min) <= 7e-3: coarse or low-wavenumber grids never do), may
 * then pass over the layers an opaque column hides from every output, wave by wave: tau and Ld keep rtx_tud's bits, Lu moves by at
 * most 2^-35 of the column's coldest Planck radiance before rounding (a few points differ by one ulp). A NaN or negative
 * depth under this flag gives undefined outputs where rtx_tud would give NaN. Every other call shape ignores the flag;
 * RADTXFR_TUD_SKIP=0 in the environment (read once) makes every call ignore it. Unknown flag bits are refused. */
#define RTX_TUD_OD_NONNEG 1u
int rtx_tud_opts(const float* OD, int64_t ld, const rtx_grid* grid, int n_layers, const double* T_h,
                 int n_alt, const uint8_t* mask_h, int n_mu, const double* mu_h, int n_down,
                 int n_angle, int return_od, float* tau, float* Lu, float* Ld, float* Ld_angles,
                 int64_t ld_out, void* stream, unsigned flags);

/* Jacobian of the rtx_tud outputs with respect to layer temperatures and mixing ratios (one slant factor mu), for the
 * layers layers_h[n_lay] (host, each in [0,n_layers), in output order):
 *   J[n_wrt][n_lay][2*n_alt+1][ld_J] float32, rows: tau of each altitude, L-up of each altitude, Ld;
 *   wrt: n_wrt = (OD_plus != NULL) + n_spec entries; T (when OD_plus is given) at position t_pos in [0, n_spec], the
 *   n_spec species of K in their order in the other positions (t_pos = 0 without OD_plus).
 * Inputs: OD[n_layers][ld] of the state; OD_plus / OD_minus[n_layers][ld] at T -+ fd_step (windows at T,
 * rtx_line_prep_window), or both NULL; K[n_spec][n_layers][ld] the optical depth per unit mixing ratio of each species;
 * tau[n_alt][ld_tau] the base transmittances rtx_tud wrote (may be NULL with return_od); T_h, mask_h, n_down, n_angle,
 * return_od as for rtx_tud. With dOD = (OD_plus - OD_minus)/(2 fd_step) for T and dOD = K for a species:
 *   J = (d row / d OD_l) dOD + [wrt = T] (d row / d T_l at fixed OD),
 * d/dOD_l of tau: -mu tau [Z_l <= zs] (return_od: mu [Z_l <= zs]); of L-up, l < count: mu t_l Q (B_l - L^(l-1)),
 * Q = prod_{l<j<count} t_j; of Ld, l < n_down: sum_q (w_q/c_q) t_{l,q} P_{l,q} (B_l - R_{l+1,q}) (P: transmittance below l,
 * R_{l+1}: downwelling radiance at the top of layer l); the fixed-OD T terms carry (1 - t) dB/dT in place of the
 * OD factor. Structural zeros (an altitude's L-up above its count, Ld above n_down, a species without lines) are exact.
 * With n_angle = 1 no stream has weight: rtx_tud's Ld is 0/0 and every Ld row of J is NaN, as its derivative is.
 * A layer's rows do not depend on which other layers are requested (bit-identical for any subset or blocking). */
int rtx_tud_jacobian(const float* OD, const float* OD_plus, const float* OD_minus, int64_t ld, double fd_step,
                     const float* K, int n_spec, const float* tau, int64_t ld_tau, const rtx_grid* grid,
                     int n_layers, const double* T_h, int n_alt, const uint8_t* mask_h, double mu, int n_down,
                     int n_angle, int return_od, const int32_t* layers_h, int n_lay, int t_pos, float* J,
                     int64_t ld_J, void* stream);
/* Adjoint of rtx_tud_jacobian (reverse mode): for n_vec cotangent vectors G on the output rows,
 *   out[v][w][k] = sum over the shard's grid->n points nu and over the rows of G[v][row][nu] * J[w][k][row][nu],
 * J exactly what rtx_tud_jacobian defines for the same arguments (all up to t_pos as there); J is never stored.
 *   G_tau, G_Lu: [n_vec][n_alt][ld_G], G_Ld: [n_vec][ld_G], float32 device arrays; each may be NULL, not all three;
 *   out: [n_vec][n_wrt][n_lay] float64 on the device, wrt slots as J's (T at t_pos).
 * A NULL row group is not evaluated: without G_Ld the downwelling stream sweeps are not run, without G_Lu and G_Ld no
 * Planck function is evaluated, without G_tau `tau` is not read (and may be NULL). With n_angle = 1 the Ld rows of J are
 * NaN: out is NaN exactly when G_Ld is given. Structural zeros of J give exact 0.0.
 * Arithmetic: the row factors are the float32 numbers rtx_tud_jacobian multiplies; every product with G and dOD/dx and
 * every sum is float64. The sum has a fixed order (64 lanes by an xor butterfly, the 4 waves of a 256-point workgroup in
 * order, the workgroups in order; no atomics): two calls give the same bits, and out[v][w][k] does not depend on the
 * other layers or vectors of the call, on their order or on how a caller blocks them.
 * n_vec is at most rtx_tud_vjp_max_vectors() (4) per call: the vectors of a call share the column sweeps, and the
 * per-workgroup staging in LDS grows with them; callers loop over groups of vectors. Scratch (one float64 per workgroup
 * and output element) is owned by the library per (device, stream). Refused: everything rtx_tud_jacobian refuses,
 * n_vec outside [1, max], ld_G < grid->n, out == NULL, all G NULL. grid->n == 0 writes zeros. */
int rtx_tud_vjp(const float* OD, const float* OD_plus, const float* OD_minus, int64_t ld, double fd_step,
                const float* K, int n_spec, const float* tau, int64_t ld_tau, const rtx_grid* grid, int n_layers,
                const double* T_h, int n_alt, const uint8_t* mask_h, double mu, int n_down, int n_angle,
                int return_od, const int32_t* layers_h, int n_lay, int t_pos, const float* G_tau,
                const float* G_Lu, const float* G_Ld, int64_t ld_G, int n_vec, double* out, void* stream);
int rtx_tud_vjp_max_vectors(void);
/* rtx_tud_jacobian and rtx_tud_vjp with the temperature derivative of the optical depths given directly:
 * dOD_dT[n_layers][ld] (rtx_voigt_sum_dt) in place of OD_plus, OD_minus and fd_step; T is always a wrt entry (at t_pos).
 * Everything else, every refusal included, as there; dOD_dT == NULL is refused. The kernels are those of the two entry
 * points above: they receive dOD_dT as OD_plus with fd_step = 1/2 and a library-owned array of n_layers * ld zeros (per
 * device, grow-only, allocated and cleared on first use: that call synchronises) as OD_minus; (D - 0) * 1 = D exactly. */
int rtx_tud_jacobian_dod(const float* OD, const float* dOD_dT, int64_t ld, const float* K, int n_spec, const float* tau,
                         int64_t ld_tau, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                         const uint8_t* mask_h, double mu, int n_down, int n_angle, int return_od,
                         const int32_t* layers_h, int n_lay, int t_pos, float* J, int64_t ld_J, void* stream);
int rtx_tud_vjp_dod(const float* OD, const float* dOD_dT, int64_t ld, const float* K, int n_spec, const float* tau,
                    int64_t ld_tau, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                    const uint8_t* mask_h, double mu, int n_down, int n_angle, int return_od, const int32_t* layers_h,
                    int n_lay, int t_pos, const float* G_tau, const float* G_Lu, const float* G_Ld, int64_t ld_G,
                    int n_vec, double* out, void* stream);
/* Tangent-linear rtx_tud (forward mode): for n_vec tangent vectors v on the wrt slots and ALL n_layers layers,
 *   out[vec][row][nu] = sum over the wrt slots w and the layers l of J[w][l][row][nu] * V_h[vec][w][l],
 * J exactly what rtx_tud_jacobian defines for the same first 18 arguments and t_pos (wrt slots as there: T at t_pos, the
 * species in K's order around it); J is never stored.
 *   V_h: [n_vec][n_wrt][n_layers] float64 on the HOST, dense; copied to a library-owned device array per (device, stream)
 *        before the call returns (the caller's array may go at once);
 *   d_tau, d_Lu: [n_vec][n_alt][ld_out], d_Ld: [n_vec][ld_out], float32 device arrays; each may be NULL, not all three.
 * A NULL row group is not evaluated and nothing is written for it: without d_Ld the downwelling stream sweeps are not
 * run, without d_Lu and d_Ld no Planck function is evaluated, without d_tau `tau` is not read (and may be NULL). With
 * n_angle = 1 the d_Ld row is NaN. Structural zeros of J give exact 0.0, and so does an all-zero vector.
 * Arithmetic: the tangents go through rtx_tud's recurrences in one pass each (O(n_layers) per point for tau and L-up,
 * O(n_layers n_angle) for Ld), dOD_l = (dOD/dT)_l v_T[l] + sum_s K_s,l v_s[l] per layer. The transmittances, Planck values,
 * dB/dT and (dOD/dT)_l are the float32 numbers rtx_tud_jacobian forms; every product with a tangent and every sum of
 * tangents is float64 in a fixed order; each output is rounded to float32 once. A point's value depends on its column and
 * on its vector alone: two calls give the same bits, and so do a shard and the same points of a larger call, a vector
 * alone and the same vector among others.
 * n_vec is at most rtx_tud_jvp_max_vectors() (4) per call: the vectors of a call share the column reads and the base
 * recurrences, and their stream tangents stay in registers; callers loop over groups of vectors. Refused: everything
 * rtx_tud_jacobian refuses about the column, n_vec outside [1, max], ld_out < grid->n, V_h == NULL, a non-finite entry of
 * V_h, all outputs NULL. grid->n == 0 returns 0 and writes nothing. rtx_tud_jvp_dod: dOD_dT in place of OD_plus, OD_minus
 * and fd_step, as rtx_tud_vjp_dod. */
int rtx_tud_jvp(const float* OD, const float* OD_plus, const float* OD_minus, int64_t ld, double fd_step,
                const float* K, int n_spec, const float* tau, int64_t ld_tau, const rtx_grid* grid, int n_layers,
                const double* T_h, int n_alt, const uint8_t* mask_h, double mu, int n_down, int n_angle,
                int return_od, int t_pos, const double* V_h, int n_vec, float* d_tau, float* d_Lu, float* d_Ld,
                int64_t ld_out, void* stream);
int rtx_tud_jvp_dod(const float* OD, const float* dOD_dT, int64_t ld, const float* K, int n_spec, const float* tau,
                    int64_t ld_tau, const rtx_grid* grid, int n_layers, const double* T_h, int n_alt,
                    const uint8_t* mask_h, double mu, int n_down, int n_angle, int return_od, int t_pos,
                    const double* V_h, int n_vec, float* d_tau, float* d_Lu, float* d_Ld, int64_t ld_out, void* stream);
int rtx_tud_jvp_max_vectors(void);
/* The tabulated G of rtx_tud, for host-side checks (no device involved): rtx_tud_gtable_size() doubles, rows of
 * {interval centre, a0 .. a6}: G(S) = sum a_k (S - centre)^k on the row's interval; intervals: 16 per binade of
 * S + 2^-6 below S = 16 (row = (bits(float(S) + 2^-6) >> 19) - (bits(2^-6) >> 19)), width 1/2 from there to S = 48.
 * g0_h receives G(0) = the sum of the quadrature weights cos(theta) sin(theta) (radiative_transfer.py:387). */
int rtx_tud_gtable_size(void);
int rtx_tud_gtable(int n_angle, double* table_h, double* g0_h);

/* compute_TUD in ONE call: radiative_transfer.py:274-392 with compute_OD (:395-456, the LBLRTM run) replaced by the
 * Voigt line-sum -- rtx_line_prep (profile Voigt, scale 1) + rtx_voigt_sum into OD[n_layers][ld_od] + rtx_tud, enqueued
 * back to back on `stream`. Arguments as for those three entry points; OD is caller-owned (it is also an output: the
 * reference's returnOD / save options expose it). One FFI crossing per atmosphere instead of three.
 * Its rtx_tud step runs as rtx_tud_opts(..., RTX_TUD_OD_NONNEG) when every weight_h, qratio_h, T_h and p_atm_h value is
 * finite and >= 0 (the optical depths are then sums of non-negative terms), as rtx_tud otherwise. The line table's own
 * strengths are not examined: a table with a negative or NaN intensity must not be combined with an opaque column. */
int rtx_compute_tud(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers,
                    const double* T_h, const double* p_atm_h, const double* qratio_h,
                    const double* weight_h, const double* mass_h, double dil_air, double dil_self,
                    double omega_wing, double omega_wing_hw, double intensity_threshold, int n_alt,
                    const uint8_t* mask_h, int n_mu, const double* mu_h, int n_down, int n_angle,
                    int return_od, float* OD, int64_t ld_od, float* tau, float* Lu, float* Ld,
                    int64_t ld_out, void* stream);
/* rtx_compute_tud with promises about what the caller does with its workspace. flags = 0 is rtx_compute_tud, launch for
 * launch. Unknown bits are refused.
 * RTX_CTUD_OD_SCRATCH: the caller will not read OD; entries no output depends on are left unwritten. Where the call is
 * eligible the layers are then summed in two launches around an early TUD launch: first layers [0, 4) and [k_top - 8,
 * n_layers), k_top = (count - 1) & ~3 with count the layers below the sensor; the TUD waves (64 consecutive points) that an
 * opaque column lets finish from those layers alone do so; then the layers in between, without those waves' rows -- a
 * line-sum tile (16 rows of 64 points) whose rows are all done returns before it loads a record; then the TUD pass of the
 * remaining waves. tau, Lu and Ld are rtx_compute_tud's bit for bit. UNSPECIFIED afterwards: OD[k][i] for k in
 * [4, k_top - 8) and i in a block of 64 points (counted from the shard's first) whose wave was done; every other entry
 * holds rtx_compute_tud's value. Which waves are done depends on the atmosphere: none in a window or a thin column.
 * Eligible: the TUD step runs the instantiation that looks for hidden layers (RTX_TUD_OD_NONNEG granted, one altitude and
 * one slant path, return_od == 0, a prefix mask, a grid fine enough for the Planck nodes, RADTXFR_TUD_SKIP not 0, the
 * default kernels); 8 <= k_top - 8; and the prologue's hot-tile bound is 0 (rtx_prep_split_bound: tables whose tiles are
 * cut into parts keep the single launch; the parts kernels take no layer subset). Every other call runs rtx_compute_tud's
 * launches and leaves OD complete. RADTXFR_OD_SKIP=0 in the environment (read once) forces that order for every call. */
#define RTX_CTUD_OD_SCRATCH 1u
int rtx_compute_tud_opts(rtx_prep* prep, const rtx_lines* lines, const rtx_grid* grid, int n_layers,
                         const double* T_h, const double* p_atm_h, const double* qratio_h,
                         const double* weight_h, const double* mass_h, double dil_air, double dil_self,
                         double omega_wing, double omega_wing_hw, double intensity_threshold, int n_alt,
                         const uint8_t* mask_h, int n_mu, const double* mu_h, int n_down, int n_angle,
                         int return_od, float* OD, int64_t ld_od, float* tau, float* Lu, float* Ld,
                         int64_t ld_out, void* stream, unsigned flags);

/* ------------------------------------------------------------------------------------------
 * At-sensor radiance. Replaces compute_LWIR_apparent_radiance(), radiative_transfer.py:1017-
 * 1069: L = tau*(emis*B(Ts+dT) + (1-emis)*Ld) + La.
 *   X[nX] fp64; emis[nX][nE]; Ts[nA] fp64; tau,La,Ld [nX][nA]; dT[nT] fp64 or NULL (nT=0)
 *   L [nX][nE][nA][max(nT,1)], Ls same shape or NULL. All spectra float32 (the reference's
 *   own caller casts to float32 first: Compute_LWIR_Apparent_Radiance.py:9-20). */
int rtx_apparent_radiance(const double* X, int64_t nX, const float* emis, int64_t nE,
                          const double* Ts, int64_t nA, const float* tau, const float* La,
                          const float* Ld, const double* dT, int64_t nT, float* L, float* Ls,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * MAKO instrument line shape. Replaces ILS_MAKO (triangle), radiative_transfer.py:1236-1256
 * (kind 0) and the Gaussian ILS_MAKO.py:21-33 (kind 1): Y_out[b][s] = sum_i w_b(X_i) Y[i][s] /
 * sum_i w_b(X_i). Band centres/widths are computed by the caller (host, :1226-1241) and passed:
 *   centre[nB] (= scale*X_out+shift), sigma[nB]: fp64 DEVICE arrays;
 *   Y [nx][nS] float32 (spectral axis first, as the reference lays it out), ldY = row stride;
 *   Y_out [nB][nS] float32. X == NULL -> uniform grid, else explicit fp64 axis (ascending). */
int rtx_ils(int kind, const rtx_grid* grid, const double* X, int64_t nx, const float* Y,
            int64_t nS, int64_t ldY, int nB, const double* centre, const double* sigma,
            float* Y_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Band averages under TABULATED spectral response functions: any sensor, not only MAKO. The
 * definition is this project's own (the reference has the two MAKO shapes only). Band b is a
 * table of knots (x_j, r_j), x strictly ascending, r finite and >= 0 (the caller checks that):
 *   R_b(x) = the piecewise-linear function through the knots, 0 outside [x_first, x_last], both
 *            ends included (two knots of value 1 are a boxcar);
 *   D_i    = the trapezoid cell of point i of the axis passed: (X[i+1] - X[i-1]) / 2 inside,
 *            half the distance to its one neighbour at either end, 1 when nx == 1;
 *   Y_out[b][s] = sum_i R_b(X_i) D_i Y[i][s]  /  sum_i R_b(X_i) D_i.
 * A band whose denominator is 0 (no axis point under it, or wholly outside the axis) comes out
 * NaN, as rtx_ils' empty band does (quirk 13), and its wsum_out is 0.
 *   X == NULL -> the uniform grid (grid->n == nx), else an explicit ascending fp64 device axis;
 *   Y [nx][nS] float32, spectral axis first, ldY = row stride;
 *   knot_start[nB + 1]: HOST, ascending; band b owns knots [knot_start[b], knot_start[b+1]),
 *     2 .. rtx_srf_max_knots() of them;  knot_x / knot_r: DEVICE, all bands' knots concatenated;
 *   Y_out [nB][nS] float32 (rtx_ils' layout);  wsum_out: NULL or [nB], the denominators.
 * Bad sizes, a NULL required pointer, ldY < nS or a bad knot_start fail before anything is launched.
 * Determinism: Y_out[b][s] is a pure function of (axis, band b's knots, column s of Y): the same
 * bits run to run, for any subset or order of the bands of a call, and for any number of columns
 * around column s (both load widths). Sums run over rows ascending inside chunks of
 * rtx_srf_chunk_points() rows cut from the axis' first point, then over the chunks ascending.
 * Calls on one stream share a grow-only workspace; only a call that grows it synchronises. */
int rtx_srf_apply(const rtx_grid* grid, const double* X, int64_t nx, const float* Y, int64_t nS,
                  int64_t ldY, int nB, const int32_t* knot_start, const double* knot_x,
                  const float* knot_r, float* Y_out, float* wsum_out, void* stream);
int rtx_srf_chunk_points(void); /* consecutive axis points one workgroup owns (for tests at the edges) */
int rtx_srf_max_knots(void);    /* largest knot count one band may have */

/* ------------------------------------------------------------------------------------------
 * Knot spectra -> monochromatic axis, column-wise np.interp. The reference's emissivity databases
 * live on ~1 cm^-1 knots (Generate_ASTER_emissivity_DB.py:48-52,81) and are resampled with
 * np.interp / interp1d before compute_LWIR_apparent_radiance (LWIR_HSI_Generator.py:151-167).
 *   Xk[nk] fp64 ascending knots; F[nk][nS] float32; out[nx][nS] float32; X == NULL -> grid.
 *   Outside [Xk[0], Xk[nk-1]] the end values are held, like np.interp. */
int rtx_interp_knots(const rtx_grid* grid, const double* X, int64_t nx, const double* Xk,
                     int64_t nk, const float* F, int64_t nS, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused at-sensor band radiances for MANY emissivity spectra given on knots (config C4):
 *   L[b][k] = ILS_b( tau*(eps_k*B(Ts) + (1-eps_k)*Ld) + La ),  eps_k = np.interp(X, Xk, E[:,k]).
 * = compute_LWIR_apparent_radiance (radiative_transfer.py:1064-1068, nA = 1, no dT) followed by
 * ILS_MAKO (:1236-1256 / ILS_MAKO.py:21-33), evaluated as (C_b + sum_j M[b][j] E[j][k]) / N_b:
 * rtx_band_moments makes ONE pass over the monochromatic tau/La/Ld (uniform grid) and writes
 *   N[nB], C[nB], M[nB][nk] float32 and jrange[nB][2] int32 (first/last knot each band touches);
 * rtx_band_mix contracts them with E[nk][nE] float32 -> out[nB][nE] float32.
 * Nothing of size nX*nE is ever formed (the reference needs a 1.4 TB temporary for this). */
int rtx_band_moments(int kind, const rtx_grid* grid, const float* tau, const float* La,
                     const float* Ld, double Ts, const double* Xk, int64_t nk, int nB,
                     const double* centre, const double* sigma, float* N_out, float* C_out,
                     float* M_out, int32_t* jrange_out, void* stream);
int rtx_band_mix(const float* N, const float* C, const float* M, const int32_t* jrange, int nB,
                 int64_t nk, const float* E, int64_t nE, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same moments for ANY sensor, and for several surface temperatures in one pass: band b is a
 * response table as rtx_srf_apply takes it, the weights are rtx_srf_apply's to the letter,
 *   w_b,i = R_b(X_i) D_i   (R_b piecewise linear through the band's knots, 0 outside, both end
 *                           knots included; D_i the trapezoid cell of the grid),
 * and with hat_j the hat functions of np.interp on Xk (end values held outside [Xk[0], Xk[nk-1]]:
 * the first and the last one extend as constants; nk == 1: one constant)
 *   N[b] = sum_i w,   C[b] = sum_i w (tau Ld + La),
 *   M[t][b][j] = sum_i w tau (B(nu_i, Ts_t) - Ld) hat_j(nu_i),   jrange[b] = first, last knot touched
 * in rtx_band_moments' conventions: rtx_band_mix(N, C, M[t], jrange, ...) gives, for temperature t,
 *   L[b][k] = sum_i w [tau (eps_k B(Ts_t) + (1 - eps_k) Ld) + La] / sum_i w,  eps_k = np.interp(X, Xk, E[:,k]).
 * Planck is evaluated at every point for every temperature (rtx_planck's constants): no node
 * interpolation, so a band may be as wide as the grid.
 *   grid: uniform only;  tau, La, Ld [grid->n] float32 DEVICE;  Xk [nk] fp64 ascending DEVICE;
 *   Ts_h [nT]: HOST, 1 <= nT <= rtx_srf_moments_max_temps(), each > 0;
 *   knot_start [nB + 1] HOST, knot_x / knot_r DEVICE: as rtx_srf_apply;
 *   N_out [nB], C_out [nB], M_out [nT][nB][nk] float32, jrange_out [nB][2] int32: DEVICE. M is written
 *   on all nk knots (0 outside jrange).
 * A band with no grid point under it has N = C = 0 and the empty range [0, -1]; rtx_band_mix then
 * divides 0 by 0: NaN, as rtx_srf_apply and rtx_ils (quirk 13). Bad sizes, a NULL required pointer,
 * a bad knot_start, nT out of range or a temperature <= 0 fail before anything is launched.
 * Determinism: N[b], C[b], M[t][b][:] and jrange[b] are a pure function of (grid, band b's knots,
 * tau, La, Ld, Xk, Ts_t): the same bits run to run, for any subset or order of the bands of a call
 * and for any subset or order of its temperatures. A sum runs over the points ascending, in fp32,
 * inside sub-chunks of 64 points cut from the grid's first point; the sub-chunk sums are added in
 * fp64 in ascending order (N and C: chunks of rtx_srf_chunk_points() points, fp64 throughout). No atomics.
 * Calls on one stream share rtx_srf_apply's grow-only workspace; only a call that grows it synchronises. */
int rtx_srf_moments(const rtx_grid* grid, const float* tau, const float* La, const float* Ld,
                    const double* Ts_h, int nT, const double* Xk, int64_t nk, int nB,
                    const int32_t* knot_start, const double* knot_x, const float* knot_r,
                    float* N_out, float* C_out, float* M_out, int32_t* jrange_out, void* stream);
int rtx_srf_moments_max_temps(void); /* temperatures one call takes */

/* ------------------------------------------------------------------------------------------
 * Adjoint of rtx_srf_moments + rtx_band_mix: from a cotangent g[t][b][e] = d cost / d L[t][b][e] on the
 * band radiances
 *   L[t][b][e] = (1 / N_b) sum_i w_b,i [tau_i (eps_e,i B(nu_i, Ts_t) + (1 - eps_e,i) Ld_i) + La_i],
 *   w, N, hat_j as at rtx_srf_moments,  eps_e,i = sum_j hat_j(nu_i) E[j][e],
 * to the native-grid cotangents rtx_tud_vjp takes and the gradients of the surface unknowns. Over
 * the live bands (N_b > 0) only:
 *   H[t][b][j] = sum_e g[t][b][e] E[j][e]
 *   A_t,i = sum_b (w_b,i / N_b) sum_j hat_j(nu_i) H[t][b][j]
 *   S_i   = sum_t sum_b (w_b,i / N_b) sum_e g[t][b][e]
 *   G_tau[i] = sum_t A_t,i (B(nu_i, Ts_t) - Ld_i) + S_i Ld_i
 *   G_La[i]  = S_i
 *   G_Ld[i]  = tau_i (S_i - sum_t A_t,i)
 *   dTs[t]   = sum_i A_t,i tau_i dB/dT(nu_i, Ts_t)       (dB/dT as rtx_tud_vjp forms it)
 *   dE[j][e] = sum_t sum_b g[t][b][e] M[t][b][j] / N_b   (M, N exactly rtx_srf_moments' outputs)
 * A band with N_b = 0 (NaN in the forward) contributes nothing, whatever its g holds, NaN included;
 * a point under no live band gets exact 0.0 in the three rows. Nothing of size nX * nE is formed.
 *   grid, tau, La, Ld, Ts_h, nT, Xk, nk, nB, knot_start, knot_x, knot_r: as rtx_srf_moments (uniform
 *     grid only, 1 <= nT <= rtx_srf_moments_max_temps());
 *   E [nk][nE] float32, g [nT][nB][nE] float32: DEVICE, nE >= 1;
 *   G_tau, G_La, G_Ld [grid->n] float32, dTs [nT] fp64, dE [nk][nE] fp64: DEVICE; any may be NULL and
 *     is then not computed (dE alone needs no pass over the points; without dE no moments are formed).
 * Everything rtx_srf_moments refuses, a NULL E or g, nE < 1 and all five outputs NULL fail before
 * anything is launched. nB == 0 writes zeros.
 * Arithmetic: w is rtx_srf_moments' fp32 weight, to the letter; N_b its chunk sums in its order,
 * rounded to fp32 as it stores them (rtx_srf_norms returns them: equal to rtx_srf_moments' N bit for
 * bit); H is an fp64 sum over e ascending, stored fp32; the hats are the forward's fp32 pair (srfm_hats);
 * S and A_t are fp64 sums over the bands in ascending band index; B and dB/dT are fp32 (planck_f32);
 * each row is formed in fp64 and rounded to fp32 once.
 * Determinism: the three rows at point i are a pure function of (grid, the bands that cover i, tau,
 * La, Ld, Xk, E, g, Ts): the same bits run to run, with bands that do not cover i added to or
 * removed from the call (band order kept), and for a shard (offset, n) of the grid that holds the
 * full support of every band covering i, its end points excluded (the trapezoid cell of a shard's
 * end point is half a cell) and its offset a multiple of rtx_srf_chunk_points() (N's chunks are cut
 * from the shard's first point; any other offset regroups an fp64 sum before its one fp32 rounding).
 * dTs: per-point fp64 terms summed by an xor butterfly over 64 lanes, then the 16 waves of a chunk in
 * wave order, then the chunks ascending. dE: fp64 over (t, b) ascending. Same bits run to run; no
 * atomics. An output's bits do not depend on which other outputs are requested.
 * Calls on one stream share a grow-only workspace; only a call that grows it synchronises. */
int rtx_srf_radiance_vjp(const rtx_grid* grid, const float* tau, const float* La, const float* Ld,
                         const double* Ts_h, int nT, const double* Xk, int64_t nk, int nB,
                         const int32_t* knot_start, const double* knot_x, const float* knot_r,
                         const float* E, int64_t nE, const float* g, float* G_tau, float* G_La,
                         float* G_Ld, double* dTs, double* dE, void* stream);
/* The denominators N[nB] float32 (DEVICE) alone, as rtx_srf_radiance_vjp forms them: equal to
 * rtx_srf_moments' N_out bit for bit. Arguments and refusals as there. */
int rtx_srf_norms(const rtx_grid* grid, int nB, const int32_t* knot_start, const double* knot_x,
                  const float* knot_r, float* N_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tangent of rtx_srf_moments + rtx_band_mix (forward mode): the change of the band radiances L of
 * rtx_srf_radiance_vjp's comment along n_vec directions in (tau, La, Ld on the native grid, the surface
 * temperatures, the emissivity knots), without a Jacobian. Per vector, with w, N, hat_j as at
 * rtx_srf_moments and tangents d_tau_i, d_La_i, d_Ld_i, dTs_t, dE[j][e]:
 *   c'_i   = d_tau_i Ld_i + tau_i d_Ld_i + d_La_i
 *   m'_t,i = d_tau_i (B(nu_i, Ts_t) - Ld_i) + tau_i (dB/dT(nu_i, Ts_t) dTs_t - d_Ld_i)
 *   C'_b = sum_i w_b,i c'_i,     M'[t][b][j] = sum_i w_b,i m'_t,i hat_j(nu_i)
 *   dL[vec][t][b][e] = (C'_b + sum_j M'[t][b][j] E[j][e] + sum_j M[t][b][j] dE[j][e]) / N_b,  j over jrange[b].
 * Nothing of size nX * nE is formed: a second set of moments with tangent integrands, then a contraction.
 *   grid, tau, Ld, Ts_h, nT, Xk, nk, nB, knot_start, knot_x, knot_r: as rtx_srf_moments (La itself is not
 *     needed), 1 <= nT <= rtx_srf_radiance_jvp_max_temps();
 *   d_tau, d_La, d_Ld: [n_vec][ld_d] float32 DEVICE (the rows rtx_tud_jvp writes), ld_d >= grid->n;
 *   dTs_h: [n_vec][nT] fp64 on the HOST, copied to a library-owned device array per (device, stream)
 *     before the call returns;  dE: [n_vec][nk][nE] float32 DEVICE;
 *   N [nB], M [nT][nB][nk], jrange [nB][2]: rtx_srf_moments' outputs for the same grid, bands, Xk and Ts_h;
 *   E [nk][nE] float32 DEVICE, nE >= 1;  dL [n_vec][nT][nB][nE] float32 DEVICE;
 *   1 <= n_vec <= rtx_srf_radiance_jvp_max_vectors(): the vectors of a call share the reads of tau and
 *     Ld, the knot search, the weights and both Planck evaluations per (point, temperature); callers
 *     loop over groups of vectors and of temperatures.
 * Any of the five tangent inputs may be NULL, not all: a NULL group is an exact zero tangent (the same
 * bits as zeros passed) and nothing is evaluated for it: without d_tau and dTs_h no Planck function,
 * without the three rows and dTs_h no pass over the points (dE alone is a contraction).
 * A band with N_b = 0 (NaN in the forward) comes out NaN. An all-zero tangent, or one that is non-zero only
 * at points under no live band, gives exact 0.0 on the live bands.
 * Refused before anything is launched, nothing written: everything rtx_srf_moments refuses, all five
 * tangent inputs NULL, n_vec or nT outside its range, ld_d < grid->n, a NULL N, M, jrange, E or dL,
 * nE < 1, a non-finite dTs_h entry. nB == 0 writes nothing and returns 0.
 * Arithmetic: c' and m' are formed in fp64 from the fp32 inputs, the fp32 B and the fp32 dB/dT
 * (rtx_tud_vjp's), left to right as written, nothing fused. w is rtx_srf_moments' fp32 weight to the
 * letter, the hats its fp32 pair (srfm_hats); every product with them, (w m') hat, is fp64 and so is every sum,
 * in a fixed order: the points ascending inside sub-chunks of 64 points cut from the grid's first point (a
 * point of weight 0 is skipped), the sub-chunks ascending; w c' over the 64 lanes of a wave by a
 * shuffle-down tree, the 16 waves of a chunk of rtx_srf_chunk_points() points in wave order, the chunks
 * ascending; the knots of jrange[b] ascending; the three terms of dL in the order written; the division
 * by the fp64 value of the caller's fp32 N; one rounding to float32, at the store. No atomics.
 * Determinism: dL[vec][t][b][:] is a pure function of (grid, band b's knots, tau, Ld, Xk, E, N[b],
 * M[t][b], jrange[b], Ts_t and vector vec's tangents): the same bits run to run, for a vector or a
 * temperature alone or among others in any order, and for any subset of the bands (order kept).
 * Calls on one stream share a grow-only workspace; only a call that grows it synchronises. */
int rtx_srf_radiance_jvp(const rtx_grid* grid, const float* tau, const float* Ld, const float* d_tau,
                         const float* d_La, const float* d_Ld, int64_t ld_d, const double* Ts_h,
                         const double* dTs_h, int nT, const double* Xk, int64_t nk, int nB,
                         const int32_t* knot_start, const double* knot_x, const float* knot_r,
                         const float* N, const float* M, const int32_t* jrange, const float* E,
                         const float* dE, int64_t nE, int n_vec, float* dL, void* stream);
int rtx_srf_radiance_jvp_max_vectors(void); /* tangent vectors one call takes */
int rtx_srf_radiance_jvp_max_temps(void);   /* temperatures one call takes */

/* ------------------------------------------------------------------------------------------
 * Fused HSI cube (config C5): every pixel has its own emissivity mixture and surface temperature
 * (LWIR_HSI_Generator.py:151-167: em = mixFrac . emis[ix_em], T = Ts + dT*N(0,1),
 * L = tau*(em*B(T) + (1-em)*Ld) + La), evaluated at monochromatic resolution and passed through
 * the ILS. B(nu, T_p) is interpolated over each band's support through Q Chebyshev nodes
 * (Q = 4: < 7e-9 relative over the MAKO bands, 230-350 K), which makes the monochromatic pass pixel-independent:
 *   rtx_band_basis_moments -> N[nB], C[nB], MLd[nB][nk], MB[Q][nB][nk], jrange[nB][2]
 *       basis_coef_h[Q][Q]: monomial coefficients of the Lagrange basis l_q(s), s = (nu-c_b)/(node_span*sigma_b)
 *       (MLd_out may be row Q of one [Q+1][nB][nk] array whose rows 0..Q-1 are MB_out)
 *   rtx_band_mix_stacked contracts the n_stack = Q+1 moment arrays M[n_stack][nB][nk] with the endmember knot
 *       spectra E[nk][nEnd] in one launch -> tab[nEnd][n_stack][nB] (bands innermost: what rtx_pixel_cube reads)
 *   rtx_pixel_cube -> cube[nB][nPix] float32 (bands first):
 *       tab[nEnd][Q+1][nB]: rows 0..Q-1 the Planck-node tables, row Q the downwelling table;
 *       kidx[nPix][nMix] int32 endmember indices, frac[nPix][nMix] float32, Tpix[nPix] fp64 (device);
 *       s_node_h[Q] the Chebyshev nodes in s. */
int rtx_band_basis_moments(int kind, const rtx_grid* grid, const float* tau, const float* La,
                           const float* Ld, const double* Xk, int64_t nk, int nB,
                           const double* centre, const double* sigma, int Q,
                           const float* basis_coef_h, double node_span, float* N_out,
                           float* C_out, float* MLd_out, float* MB_out, int32_t* jrange_out,
                           void* stream);
int rtx_band_mix_stacked(const float* M, const int32_t* jrange, int nB, int n_stack, int64_t nk,
                         const float* E, int64_t nE, float* tab, void* stream);
int rtx_pixel_cube(int nB, int Q, const double* centre, const double* sigma, double node_span,
                   const float* s_node_h, const float* N, const float* C, const float* tab,
                   int nEnd, int64_t nPix, int nMix, const int32_t* kidx, const float* frac,
                   const double* Tpix, float* cube, void* stream);

/* ------------------------------------------------------------------------------------------
 * The HSI cube for ANY sensor: bands are response tables as rtx_srf_moments takes them, of any width.
 * The definition is this project's own (the reference has the MAKO shapes only). B(nu, T_p) is
 * interpolated IN TEMPERATURE through Q nodes T_q of the scene's range [T_lo, T_hi] (rtx_pixel_cube
 * interpolates in wavenumber across a band, which holds for MAKO-narrow bands only):
 *   N, C, M[q], jrange = rtx_srf_moments at Ts = the Q nodes, unchanged, in one call
 *   G[e][q][b]  = sum_{j in jrange[b]} M[q][b][j] E[j][e]                          (rtx_srf_cube_tables)
 *   l_q(T)      = prod_{r != q} (T - T_r) / prod_{r != q} (T_q - T_r)
 *   cube[b][p]  = ( C_b + sum_m frac[p][m] sum_q l_q(T_p) G[kidx[p][m]][q][b] ) / N_b  (rtx_srf_pixel_cube)
 * The Ld term inside M rides through exactly (sum_q l_q = 1). No Planck function is evaluated per pixel.
 *   rtx_srf_cube_max_nodes() = 8 = rtx_srf_moments_max_temps().
 *   rtx_srf_cube_tables: M [Q][nB][nk], jrange [nB][2], E [nk][nEnd] float32 -> tab [nEnd][Q][nB] (bands
 *     innermost), all DEVICE; one fp32 fmaf chain per entry over the knots of jrange[b] ascending.
 *     Refused before the launch: Q outside [1, max_nodes], nk < 1, a negative size, a NULL pointer;
 *     nB == 0 or nEnd == 0 writes nothing and returns 0.
 *   rtx_srf_pixel_cube: T_node_h on the HOST, Q + 2 values: the Q nodes, strictly monotonic, then T_lo
 *     and T_hi, the range the interpolant is admitted on, T_lo <= every node <= T_hi (Chebyshev nodes lie
 *     inside their range, so the range is not the nodes' hull and travels with them);
 *     N [nB], C [nB], tab [nEnd][Q][nB] float32; kidx [nPix][nMix] int32, frac [nPix][nMix] float32,
 *     Tpix [nPix] fp64: DEVICE; cube [nB][nPix] float32 DEVICE.
 *     A band with N_b = 0 comes out NaN in every pixel (quirk 13). A pixel whose temperature is not
 *     finite or lies outside [T_lo, T_hi] is NaN down its whole column: no extrapolation, and no
 *     device-to-host check. An endmember index outside [0, nEnd) is clamped, as rtx_pixel_cube does.
 *     Refused before the launch, nothing written: a NULL required pointer, Q outside [1, max_nodes], a node
 *     or range end that is not finite, not positive, outside the range or not distinct from another node,
 *     nEnd < 1, nMix < 1, a negative size. nB == 0 or nPix == 0 writes nothing and returns 0.
 * Arithmetic: l_q(T_p) once per pixel: numerator and denominator are fp64 products over r ascending, one
 * fp64 division, one rounding to fp32 (a pixel exactly at a node gets the weights 1 and 0 exactly). Then
 * fp32:  s = 0;  for m ascending { t = 0; for q ascending t = fmaf(l_q, G[k_m][q][b], t); s = fmaf(frac_m, t, s); }
 * cube = (C_b + s) / N_b.
 * Determinism: cube[b][p] is a pure function of (pixel p's kidx, frac and T; band b's N, C and tab
 * column; the nodes and the range): the same bits run to run, for any nPix, for any position of the
 * pixel in the scene, for any subset of the bands (order kept), and whether the kernel holds the table
 * in LDS (nEnd * Q <= 128) or reads it from global memory. No atomics, no workspace. */
int rtx_srf_cube_max_nodes(void);
int rtx_srf_cube_tables(const float* M, const int32_t* jrange, int nB, int Q, int64_t nk,
                        const float* E, int64_t nEnd, float* tab, void* stream);
int rtx_srf_pixel_cube(int nB, int Q, const double* T_node_h, const float* N, const float* C,
                       const float* tab, int nEnd, int64_t nPix, int nMix, const int32_t* kidx,
                       const float* frac, const double* Tpix, float* cube, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adjoint of rtx_srf_pixel_cube: J^T g for the pixels' temperatures and fractions and for the band
 * radiances of the pure endmembers at the nodes, without a Jacobian and without anything of size
 * nPix x nX or nPix x nk. With N, tab = G and l_q as above the cube is a linear combination of band
 * radiances,
 *   cube[b][p] = sum_m f_pm sum_q l_q(T_p) L[q][b][k_pm] + (1 - sum_m f_pm) L0[b],
 *   L[q][b][e] = (C_b + G[e][q][b]) / N_b,   L0[b] = C_b / N_b   (emissivity 0; sum_q l_q = 1),
 * so with u_bp = g[b][p] on a live band (N_b > 0) and an admitted pixel (T_p finite and inside
 * [T_lo, T_hi]) and u_bp = 0 otherwise -- a select, not a product: a NaN in g under a dead band or a
 * refused pixel does not spread --
 *   dfrac[p][m] = sum_b (u_bp / N_b) sum_q l_q(T_p)  G[k_pm][q][b]
 *   dT[p]       = sum_b (u_bp / N_b) sum_m f_pm sum_q l'_q(T_p) G[k_pm][q][b]
 *   gL[q][b][e] = sum_p u_bp l_q(T_p) sum_{m: k_pm = e} f_pm                      (e < nEnd)
 *   gL[0][b][nEnd] = sum_p u_bp (1 - sum_m f_pm),  gL[q > 0][b][nEnd] = 0         (the cotangent of L0)
 * with l'_q(T) = sum_{s != q} prod_{r != q, s} (T - T_r) / den_q and k_pm clamped to [0, nEnd) as the
 * forward clamps it. gL [Q][nB][nEnd + 1] is the cotangent rtx_srf_radiance_vjp takes with Ts = the Q
 * nodes and E' = [E | 0] (one added column of zero emissivity): its rows are G_tau / G_La / G_Ld of the
 * cube, the first nEnd columns of its dE the gradient of the endmember knots.
 *   nB, Q, T_node_h, N, tab, nEnd, nPix, nMix, kidx, frac, Tpix: as rtx_srf_pixel_cube (C is not needed);
 *   g [nB][nPix] float32 DEVICE; dT [nPix] fp64, dfrac [nPix][nMix] fp64, gL [Q][nB][nEnd + 1] float32
 *   DEVICE, each may be NULL (not computed), not all three.
 * A pixel that is not admitted gets NaN in its own dT and dfrac (the forward gave it a NaN column) and
 * adds exact zeros to gL; a dead band adds nothing anywhere.
 * Refused before anything is launched, nothing written: everything rtx_srf_pixel_cube refuses, a NULL g,
 * all three outputs NULL, flags != 0. nB == 0 or nPix == 0 writes zeros to the outputs given and returns 0.
 * Arithmetic: l_q and l'_q in fp64 from the nodes and the host's denominators, products over r
 * ascending (l'_q: the sum over s ascending of such products), one fp64 division, one rounding to fp32:
 * l_q has rtx_srf_pixel_cube's bits, so a pixel on a node has the weights 1 and 0. The inner sums over q
 * are fp32 fmaf chains over the table, q ascending: t = sum_q l_q G, t' = sum_q l'_q G. Everything after
 * that is fp64: x = (double)u * (1 / (double)N_b); dfrac's term x t; dT's term x sum_m f_m t'_m (m
 * ascending, each product exact); gL's term u (l_q f_m) (the inner product exact). A mixture of more
 * than 4 is taken 4 slots at a time and dT adds the passes' band sums in pass order. gL is rounded to
 * fp32 once, at the store. No atomics.
 * Determinism: dT[p] and dfrac[p][:] are pure functions of (pixel p's kidx, frac, T and column of g; the
 * bands; the nodes and the range): the same bits for any nPix, any position of the pixel in the scene,
 * whatever other outputs are asked for, and whether the table slice is held in LDS (nEnd * Q <= 128) or
 * read from global memory. The sum over the bands runs over the 64 lanes of a block of 64 bands along the
 * xor tree of rtx_srf_radiance_vjp's dTs sum (distance 1, 2, 4, .. 32), then over the blocks ascending.
 * gL has the same bits run to run for a given scene: within a chunk of pixels a table row takes its
 * pixels ascending (a pixel's slots ascending; a mixture of more than 8 is taken 8 slots at a time per
 * group of 64 pixels), then the chunks are added ascending; a chunk is 256 pixels, doubled until the
 * chunk sums ([chunks][nEnd + 1][Q][nB] fp64) fit 64 MiB. Calls on one stream share a grow-only
 * workspace, owned per (device, stream); a call that has to grow it waits for the device first.
 * flags: none is defined, pass 0 (anything else is refused). */
int rtx_srf_pixel_cube_vjp(int nB, int Q, const double* T_node_h, const float* N, const float* tab,
                           int nEnd, int64_t nPix, int nMix, const int32_t* kidx, const float* frac,
                           const double* Tpix, const float* g, double* dT, double* dfrac, float* gL,
                           void* stream, unsigned flags);

/* ------------------------------------------------------------------------------------------
 * Tangent of rtx_srf_pixel_cube: J v along directions in the pixels' fractions and temperatures and in
 * the band radiances of the pure endmembers at the nodes, without a Jacobian; the exact transpose of
 * rtx_srf_pixel_cube_vjp. With N, tab = G, l_q, l'_q, L and the clamped k_pm as there, per vector v
 *   t_m  = sum_q l_q(T_p)  G[k_pm][q][b]
 *   t'_m = sum_q l'_q(T_p) G[k_pm][q][b]
 *   s_m  = sum_q l_q(T_p)  dL[v][q][b][k_pm]
 *   d_cube[v][b][p] = sum_m ( d_frac[v][p][m] t_m + d_Tpix[v][p] frac[p][m] t'_m ) / N_b
 *                   + sum_m frac[p][m] s_m + (1 - sum_m frac[p][m]) dL[v][0][b][nEnd]
 * dL [n_vec][Q][nB][nEnd + 1] is the tangent of L: what rtx_srf_radiance_jvp writes at Ts = the Q nodes,
 * E' = [E | 0], dE' = [dE | 0], no dTs (its column nEnd holds the same bits at every node; node 0's is
 * taken, where the adjoint places the cotangent). The d_Tpix term is the derivative of the interpolant
 * rtx_srf_pixel_cube evaluates, not of Planck's function.
 *   nB, Q, T_node_h, N, tab, nEnd, nPix, nMix, kidx, frac, Tpix: as rtx_srf_pixel_cube_vjp;
 *   d_frac [n_vec][nPix][nMix] float32, d_Tpix [n_vec][nPix] fp64, dL float32: DEVICE, each may be NULL
 *   (an exact zero tangent: nothing is read or evaluated for it, and the result has the bits of zeros
 *   passed), not all three; 1 <= n_vec <= rtx_srf_pixel_cube_jvp_max_vectors() = 2;
 *   d_cube [n_vec][nB][nPix] float32 DEVICE.
 * A band with N_b = 0 is NaN in every pixel and a pixel whose temperature is not finite or lies outside
 * [T_lo, T_hi] is NaN down its column, in every vector: selects at the store, whatever the tangents hold.
 * Refused before anything is launched, nothing written: everything rtx_srf_pixel_cube refuses, all three
 * tangents NULL, a NULL d_cube, n_vec outside [1, max_vectors], flags != 0. nB == 0 or nPix == 0 writes
 * nothing and returns 0.
 * Arithmetic: l_q and l'_q as rtx_srf_pixel_cube_vjp forms them (the same code). t, t' and s are fp32
 * fmaf chains, q ascending: t and t' have the adjoint's bits. Then fp64, m ascending:
 *   A = fma(d_frac, t, A);  A = fma(d_Tpix * frac, t', A);  B = fma(frac, s, B);  F = F + frac
 *   d_cube = fma(1 - F, dL[v][0][b][nEnd], A / (double)N_b + B), rounded to float32 once, at the store.
 * Determinism: d_cube[v][b][p] is a pure function of (pixel p's kidx, frac, T, d_frac[v] and d_Tpix[v];
 * band b's N and tab column; vector v's dL column; the nodes and the range): the same bits run to run,
 * for any nPix, any position of the pixel in the scene, any subset of the bands (order kept), for a
 * vector alone or beside another, and whether the table slice is held in LDS (nEnd * Q <= 128) or read
 * from global memory. No atomics. The vectors of a call share the pixel's weights, its mixture and t,
 * t'; each has one 16 KiB output tile in LDS beside at most 32 KiB of table, which is what bounds
 * max_vectors. dL is re-laid with the bands innermost into a grow-only workspace, owned per (device,
 * stream), that also holds the weights; a call that has to grow it waits for the device first.
 * flags: none is defined, pass 0 (anything else is refused). */
int rtx_srf_pixel_cube_jvp(int nB, int Q, const double* T_node_h, const float* N, const float* tab,
                           int nEnd, int64_t nPix, int nMix, const int32_t* kidx, const float* frac,
                           const double* Tpix, const float* d_frac, const double* d_Tpix,
                           const float* dL, int n_vec, float* d_cube, void* stream, unsigned flags);
int rtx_srf_pixel_cube_jvp_max_vectors(void);

/* ------------------------------------------------------------------------------------------
 * Per-pixel least-squares fit of temperature and fractions to a measured cube. The
 * atmosphere (N, C, tab) and every pixel's endmember indices are fixed, so each pixel is its own
 * problem in the 1 + nMix unknowns u = (T, f_1 .. f_nMix), in that order, under rtx_srf_pixel_cube's
 * model y_b(u). N, C, tab = G, the nodes, the range, l_q, l'_q, the clamped k_pm, "live band" (N_b > 0)
 * and "admitted pixel" (T finite and inside [T_lo, T_hi]) are as in rtx_srf_pixel_cube / _vjp.
 *   meas [nB][nPix] float32 DEVICE: the measured cube, in the forward's layout;
 *   wgt  [nB] float32 DEVICE or NULL (every weight 1). A band COUNTS when it is live and w_b > 0: a select,
 *   so whatever meas holds under a band that does not count (NaN included) is never read.
 * One evaluation at u (T fp64, f float32 as the forward takes them), per counting band:
 *   w_q = (float)l_q, w'_q = (float)l'_q, by the adjoint's code (l_q has the forward's bits);
 *   t_m = fmaf(w_q, G[k_m][q][b], t_m), t'_m = fmaf(w'_q, G[k_m][q][b], t'_m), q ascending (fp32);
 *   s = fmaf(f_m, t_m, s), m ascending;  y = (C_b + s) / N_b in fp32: rtx_srf_pixel_cube's bits;
 *   then fp64: r = (double)y - (double)meas, invN = 1 / (double)N_b,
 *   j_0 = invN * S with S = fma((double)f_m, (double)t'_m, S), m ascending;  j_m = invN * (double)t_m;
 *   wr = w r;  cost = fma(wr, r, cost);  grad_i = fma(j_i, wr, grad_i);  H_ij = fma(w j_i, j_j, H_ij), i >= j.
 * THE BAND SUM RUNS OVER THE BANDS ASCENDING, in the pixel's own lane, wherever the table lies.
 *   cost = sum w r^2 (no 1/2), grad = J^T W r, H = J^T W J packed as the lower triangle by rows
 *   (H_00, H_10, H_11, H_20, ..): (1 + nMix)(2 + nMix) / 2 values.
 * Damped step: (H + lambda diag H) step = -grad by Cholesky in fp64, A_ii = fma(lambda, H_ii, H_ii), the
 * columns ascending, every inner sum by fma(-L_ik, L_jk, .) with k ascending, forward then back
 * substitution. A pivot that is not finite or not positive: the step is NaN ("singular").
 *
 * rtx_srf_pixel_cube_normal: one evaluation at (Tpix, frac) and one step per pixel.
 *   lambda [nPix] fp64 DEVICE or NULL (0); cost [nPix] fp64; grad [nPix][1 + nMix], hess
 *   [nPix][(1 + nMix)(2 + nMix) / 2], step [nPix][1 + nMix] fp64 DEVICE, each may be NULL (not written).
 *   A pixel that is not admitted gets NaN in all its outputs. flags: none is defined, pass 0.
 * rtx_srf_pixel_cube_fit: Levenberg-Marquardt per pixel; pixels never interact.
 *   1 start: under RTX_FIT_START_GIVEN the (Tpix, frac) passed in. Otherwise the node scan: for q ascending,
 *     T = T_q (the weights are exactly 1 and 0); evaluate at f = 0; f_q = (float)(-H_ff^-1 grad_f), the
 *     fraction block alone with lambda = 0 (a singular block skips the node); evaluate at (T_q, f_q); the
 *     strictly smallest cost is kept, the first node wins a tie. No node with a finite cost, or a given
 *     start whose cost is not finite: status 3.
 *   2 lambda = lambda0.
 *   3 a trial: the step; T' = min(max(T + step_0, T_lo), T_hi); f'_m = (float)((double)f_m + step_m);
 *     evaluate at u'; accepted iff cost' < cost (a NaN cost rejects). Accepted: lambda = max(0.1 lambda,
 *     1e-12), the trial's H and grad become current. Rejected: lambda = min(10 lambda, 1e12). n_iter counts
 *     trials.
 *   4 stops, tested in this order before a trial: cost == 0 (status 0); n_iter == max_iter (status 1); a
 *     singular step (status 3). After an accepted trial: cost - cost' < ftol cost (status 0; ftol = 0:
 *     never). After a rejected one: lambda at its cap (status 0).
 *   5 status [nPix] int32: 0 stopped by cost, ftol or the cap of lambda; 1 iteration cap; 2 the given start
 *     is not admitted or a fraction of it is not finite; 3 singular. Under 2 and 3 Tpix, frac, cost and
 *     hess of the pixel are NaN.
 *   frac [nPix][nMix] float32 and Tpix [nPix] fp64 DEVICE: read under RTX_FIT_START_GIVEN, always written;
 *   0 <= max_iter <= rtx_srf_pixel_cube_fit_max_iter() = 1000, so every launch terminates; lambda0 and
 *   ftol finite and >= 0; cost [nPix] fp64, n_iter [nPix] int32; hess as above, the final point's, or NULL.
 * Both: 1 <= nMix <= rtx_srf_pixel_cube_fit_max_mix() = 4 (what every instantiation holds in registers
 * without scratch). Refused before anything is launched, nothing written: everything rtx_srf_pixel_cube
 * refuses, a NULL meas or required output, nMix above max_mix, max_iter outside its range, lambda0 or
 * ftol not finite or negative, unknown flag bits. nB == 0 or nPix == 0 writes nothing and returns 0.
 * Determinism: every output of pixel p is a pure function of (pixel p's kidx, start and column of meas;
 * the counting bands and wgt; the nodes and the range): the same bits run to run, for any nPix, any
 * position of the pixel in the scene, for the table slice in LDS (nEnd * Q <= 128) or read from global
 * memory, and in _normal whichever optional outputs are asked for. _fit under RTX_FIT_START_GIVEN equals,
 * bit for bit, a host loop over _normal that applies rule 3 in fp64. Lane = pixel: no atomics, no
 * cross-lane sum, no workspace. */
#define RTX_FIT_START_GIVEN 1u
int rtx_srf_pixel_cube_fit_max_mix(void);
int rtx_srf_pixel_cube_fit_max_iter(void);
int rtx_srf_pixel_cube_normal(int nB, int Q, const double* T_node_h, const float* N, const float* C,
                              const float* tab, int nEnd, int64_t nPix, int nMix, const int32_t* kidx,
                              const float* frac, const double* Tpix, const float* meas, const float* wgt,
                              const double* lambda, double* cost, double* grad, double* hess, double* step,
                              void* stream, unsigned flags);
int rtx_srf_pixel_cube_fit(int nB, int Q, const double* T_node_h, const float* N, const float* C,
                           const float* tab, int nEnd, int64_t nPix, int nMix, const int32_t* kidx,
                           const float* meas, const float* wgt, float* frac, double* Tpix, int max_iter,
                           double lambda0, double ftol, double* cost, int32_t* n_iter, int32_t* status,
                           double* hess, void* stream, unsigned flags);

/* ------------------------------------------------------------------------------------------
 * The same fit inside a box: T_lo <= T <= T_hi, f_m >= 0, and an optional soft sum-to-one.
 * Unknowns, model, meas, wgt, counting bands, one evaluation and the packing of H are those above; what
 * rtx_srf_pixel_cube_normal and rtx_srf_pixel_cube_fit compute does not change.
 * The pseudo-band: with sum_weight = delta > 0 (fp64; delta == 0 skips it entirely) one more term follows
 * the band loop, accumulated exactly as a band:
 *   r_s = (sum_m (double)f_m, m ascending, plain fp64 adds) - 1,  j_0 = 0,  j_m = 1;
 *   cost = fma(delta r_s, r_s, cost);  grad_m = fma(1, delta r_s, grad_m);  H_mm' = fma(delta, 1, H_mm'), m, m' >= 1.
 * delta weighs (sum f - 1)^2 against squared radiance residuals: its unit is radiance^2, and delta =
 * (sigma_L / sigma_sum)^2 asks the sum to stay within sigma_sum of 1 beside a band noise of sigma_L.
 * The box step from u = (T, (double)f_1 ..) with grad g, H, lambda, lo = (T_lo, 0, ..), hi = (T_hi, +inf, ..):
 *   1 B = { i : (u_i <= lo_i and g_i > 0) or (u_i >= hi_i and g_i < 0) }, with prescribed steps s_i = 0.
 *   2 a pass: the Cholesky solve above, same order and fma pattern, over all 1 + nMix unknowns of the matrix
 *     whose rows and columns of B are the identity's (A_ii = 1, undamped, off-diagonals 0; the L entries there
 *     are exact zeros, so the free block has the bits of its own Cholesky), A_jj = fma(lambda, H_jj, H_jj) on
 *     the free diagonal. Right-hand side: s_i on B; for a free j, -(g_j + sum_{i in B} H_ji s_i), the sum by
 *     fma(H_ji, s_i, .) onto g_j with i ascending. d_i = s_i on B. Every free i with u_i + d_i < lo_i joins B
 *     with s_i = lo_i - u_i, with u_i + d_i > hi_i with s_i = hi_i - u_i. None joined: the step is d.
 *     Otherwise another pass, 1 + nMix passes at most; what joins in the last one was the only free unknown
 *     left and takes d_i = s_i. A pivot that is not finite or not positive in any pass: the step is NaN.
 *   3 the trial point: T' = min(max(T + d_0, T_lo), T_hi); f'_m = max(0f, (float)((double)f_m + d_m)), where
 *     max(0f, x) = x > 0 ? x : 0f.
 * rtx_srf_pixel_cube_normal_box: rtx_srf_pixel_cube_normal's arguments, then sum_weight and
 *   active [nPix] int32 DEVICE or NULL: bit i set where unknown i ended in B (step 1's set included); 0 for a
 *   pixel that is not admitted. step is the box step d; cost, grad and hess include the pseudo-band. With
 *   sum_weight == 0, at a point strictly inside the box whose step stays inside, every output has
 *   rtx_srf_pixel_cube_normal's bits.
 * rtx_srf_pixel_cube_fit_box: rtx_srf_pixel_cube_fit's arguments, then sum_weight,
 *   grad [nPix][1 + nMix] fp64 DEVICE or NULL: the final point's gradient (NaN under status 2 and 3), and
 *   active [nPix] int32 DEVICE or NULL: step 1's set at the final point, the KKT active set (0 under status 2
 *   and 3). The covariance of the free unknowns is the inverse of hess with those rows and columns removed.
 *   Rules 1 - 5 of rtx_srf_pixel_cube_fit with these changes: a given start's fractions are projected by
 *   max(0f, .) first (status 2 is decided on the values passed in); the node scan's second evaluation is at
 *   the trial point of the box step with T held in B (s_0 = 0), lambda = 0, from (T_q, f = 0), and a NaN step
 *   skips the node; a trial is the box step and its trial point; and one more stop, tested after the singular
 *   step and before the evaluation: a trial point equal bit for bit to the current point gives status 0 and
 *   is not counted in n_iter. The accept rule, the lambda schedule, caps, statuses and NaN rules are unchanged.
 * Both: 1 <= nMix <= rtx_srf_pixel_cube_fit_box_max_mix() = 4 (every instantiation without scratch). Refused
 * before anything is launched, nothing written: everything the unconstrained entries refuse, and a
 * sum_weight that is not finite or negative. nB == 0 or nPix == 0 writes nothing and returns 0 (with no band
 * the pseudo-band is not evaluated either).
 * Determinism: every output of pixel p is a pure function of (pixel p's kidx, start and column of meas;
 * the counting bands and wgt; the nodes and the range; sum_weight): the same bits run to run, for any nPix,
 * any position of the pixel in the scene, for the table slice in LDS (nEnd * Q <= 128) or read from global
 * memory, and in _normal_box whichever optional outputs are asked for. _fit_box under RTX_FIT_START_GIVEN
 * equals, bit for bit, a host loop over _normal_box that applies rule 3 and the new stop in fp64. Lane =
 * pixel: no atomics, no cross-lane sum, no workspace. */
int rtx_srf_pixel_cube_fit_box_max_mix(void);
int rtx_srf_pixel_cube_normal_box(int nB, int Q, const double* T_node_h, const float* N, const float* C,
                                  const float* tab, int nEnd, int64_t nPix, int nMix, const int32_t* kidx,
                                  const float* frac, const double* Tpix, const float* meas, const float* wgt,
                                  const double* lambda, double* cost, double* grad, double* hess,
                                  double* step, void* stream, unsigned flags, double sum_weight,
                                  int32_t* active);
int rtx_srf_pixel_cube_fit_box(int nB, int Q, const double* T_node_h, const float* N, const float* C,
                               const float* tab, int nEnd, int64_t nPix, int nMix, const int32_t* kidx,
                               const float* meas, const float* wgt, float* frac, double* Tpix, int max_iter,
                               double lambda0, double ftol, double* cost, int32_t* n_iter, int32_t* status,
                               double* hess, void* stream, unsigned flags, double sum_weight, double* grad,
                               int32_t* active);

/* ------------------------------------------------------------------------------------------
 * Speed-dependent Voigt line-sum. Replaces the per-line PROFILE_SDVOIGT + scatter-add of
 * absorptionCoefficient_SDVoigt, misc/hapi.py:10897-10900 (PROFILE_SDVOIGT :10117 -> pcqsdhc :9850-10024 with
 * anuVC = eta = 0: PART1 for lines without speed dependence, PART2/3/4 otherwise; CPF = hum1_wei :9833, cpf3 :9645),
 * after rtx_line_prep_profile(..., RTX_PROFILE_SDVOIGT, ...). Evaluated in fp64 (the profile is a difference of two
 * complex probability functions): a workgroup per tile of 1024 points, far wings at Chebyshev nodes (32 per tile / 12 per
 * 64-point row, interpolation <= 1e-10 of a line's own contribution), the rows around a centre and around every regime
 * switch point by point; RADTXFR_SD_KERNEL=gather selects the one-thread-per-point cross-check. This is the
 * cross-section generator's path (misc/RT_gen_AbsXS_files.py:90), not the TUD hot path.
 *   out_f32[n_layers][ld] (may be NULL)  (float)(sum * scale);  out_f64[n_layers][ld] (may be NULL)  sum */
int rtx_sdvoigt_sum(const rtx_prep* prep, const rtx_grid* grid, int n_layers, float* out_f32,
                    double* out_f64, int64_t ld, void* stream);

/* ---- hapi's line-profile functions with explicit parameters --------------------------------------------------
 * Replace pcqsdhc / PROFILE_HT(P) / PROFILE_SDRAUTIAN / PROFILE_RAUTIAN / PROFILE_SDVOIGT / PROFILE_VOIGT, PROFILE_LORENTZ
 * and PROFILE_DOPPLER (misc/hapi.py:9850-10160) and the complex probability functions hum1_wei (:9833) and cpf3 (:9645),
 * as people who fit spectra call them: per-line parameters, no line table, no environment, no windows. fp64 throughout.
 * The profile is the COMPLETE pcqsdhc: PART1 (Aterm; Bterm for |Z1| <= 4000 and beyond), PART2, PART3 (|sqrt X| <= 4000
 * and beyond), PART4 (with the cpf3 shell) and the common part (1/pi) A / (1 - (anuVC - eta (c0 - 1.5 c2)) A + eta c2 B),
 * eta complex, real and imaginary part. Each point is what the reference returns for that point ALONE, sg = array([s])
 * (its vector call needs every point of a call in one PART); PART3's far form uses PART3's own W (the reference raises
 * there). Parameters are not validated (GamD = 0, eta = 1: what IEEE arithmetic gives). DESIGN.md section 4.14.
 *   params[n_lines][10] fp64, device: sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, Re eta, Im eta, pad.
 *   sg[n] fp64, device: the points, in any order, repeats allowed.
 *   rtx_profile_eval  every line at every point: out_re / out_im [n_lines][ld] (out_im may be NULL). kind:
 *       RTX_LS_PCQSDHC  the profile above;
 *       RTX_LS_LORENTZ  Gam0 / (pi (Gam0^2 + (sg - sg0)^2)), :10150 (reads sg0, Gam0);
 *       RTX_LS_DOPPLER  cSqrtLn2divSqrtPi exp(-cLn2 ((sg - sg0) / GamD)^2) / GamD with hapi's rounded constants, :10160
 *                       (reads sg0, GamD). Both are real: out_im, when given, is set to 0.
 *       A point's value is a function of (its line's parameters, sg) alone: bit-identical wherever it stands in sg.
 *   rtx_profile_sum   out[i] = sum_l w_re[l] Re LS_l(sg[i]) + w_im[l] Im LS_l(sg[i]), pcqsdhc: the model spectrum of a fit
 *       (strengths on the real part, first-order mixing coefficients times strengths on the imaginary part). w_re / w_im
 *       [n_lines] fp64, device; w_im may be NULL (= 0). One thread per point, lines in index order, one association
 *       (acc = acc + (w_re Re + w_im Im)): bit-reproducible, and independent of n and of the order of sg.
 *   rtx_cpf_eval      out[i] = hum1_wei(x[i], y[i]) (RTX_CPF_HUM1_WEI: Weideman-24 inside |x| + y < 15, the one-term
 *       asymptote outside; y may be negative; |z| < 1e154, where (L - iz)^2 overflows as in the reference) or cpf3(x[i], y[i]) (RTX_CPF_CPF3: the 15-term series, meant for |z| ~ 8;
 *       1/z by a Newton-refined reciprocal, so 1e-150 < |z| < 1e150); out_im may be NULL.
 * Errors (before any device work): a required pointer NULL, a negative count, ld < n, an unknown kind. n = 0 or
 * n_lines = 0 succeeds without a launch and writes nothing. Asynchronous on `stream`; nothing is allocated. */
#define RTX_LS_PCQSDHC 0
#define RTX_LS_LORENTZ 1
#define RTX_LS_DOPPLER 2
#define RTX_CPF_HUM1_WEI 0
#define RTX_CPF_CPF3 1
int rtx_profile_eval(int kind, int64_t n_lines, const double* params, const double* sg, int64_t n,
                     double* out_re, double* out_im, int64_t ld, void* stream);
int rtx_profile_sum(int64_t n_lines, const double* params, const double* w_re, const double* w_im,
                    const double* sg, int64_t n, double* out, void* stream);
int rtx_cpf_eval(int kind, const double* x, const double* y, int64_t n, double* out_re,
                 double* out_im, void* stream);

/* ---- Hartmann-Tran line-sum on a line table ---------------------------------------------------------------------
 * Replaces the per-line block and the scatter-add of absorptionCoefficient_HT, misc/hapi.py:10474-10651, for tables that
 * carry Hartmann-Tran columns: the HT-named lookups with their fallbacks to the Voigt-style columns, PROFILE_HT (the
 * pcqsdhc of rtx_profile_eval) on each line's window, summed in fp64. DESIGN.md section 4.15.
 *
 * rtx_lines_set_ht: the HT columns of n_sets broadener column sets. set_h[n_sets] = column set of each (0 air, 1 self,
 * 2 + j extra set j of rtx_lines_set_broadeners, which must have been called first); cols_h[n_sets][RTX_HT_COLS] = host
 * pointers to columns of n_lines doubles in the row order of rtx_lines_create, NULL = absent, in this order:
 *   slots 6 b + 0 .. 6 b + 5 for TrefHT bucket b = 0, 1, 2, 3 (50, 150, 296, 700 K):
 *       gamma_HT_0_<sp>_<Tref>, n_HT_<sp>_<Tref>, gamma_HT_2_<sp>_<Tref>, delta_HT_0_<sp>_<Tref>, deltap_HT_<sp>_<Tref>,
 *       delta_HT_2_<sp>_<Tref>;
 *   slots 24, 25, 26: nu_HT_<sp>, kappa_HT_<sp>, eta_HT_<sp>.
 * An absent column and a column of zeros behave the same (the reference's try / except, :10505-10637). Replaces the table's
 * previous HT sets; n_sets = 0 drops them. Allocates device memory and synchronises.
 *
 * rtx_ht_create: an object for tables of n_lines lines, up to max_states states and axes of up to max_points points. It
 * holds no device memory until the first rtx_ht_prep with work to do (which allocates, hence synchronises, once).
 *
 * rtx_ht_prep: per (line, state), fp64. X_h[nx]: the axis, host, finite and non-decreasing (repeats allowed, nx = 1
 * allowed), copied to the device. T_h, p_atm_h, qratio_h, weight_h, mass_h, n_dil, dil_h, frac_h, omega_wing, omega_wing_hw,
 * intensity_threshold, scale: as rtx_line_prep_mix (frac_h[n_dil][n_species][n_states]). For each line
 *   S(T) = sw qratio ch(T) / ch(296 K); weight = 0 or S < intensity_threshold drops the line;
 *   TrefHT = 50 / 150 / 296 / 700 K for T in [0,100) / [100,200) / [200,400) / otherwise (:10394-10398);
 *   per diluent, in the caller's order (a set may repeat): each parameter from its HT column of that bucket, or from the
 *   Voigt-style column of the set where the HT value is 0 (self n = 0 and an absent n: n_air; Gamma2: SD * gamma);
 *   Gamma0 from the Tref of the n lookup, Shift0 and NuVC from the Tref of the deltap lookup; Gamma2, Shift2 times p;
 *   Eta = sum EtaDB abun (Gamma0T + i Shift0T) / (Gamma0 + i Shift0);
 *   window [bisect_right(X, nu - W), bisect_right(X, nu + W)), W = max(omega_wing, omega_wing_hw Gamma0, omega_wing_hw GammaD).
 * rtx_ht_sum: out[k][i] = sum over lines, in line order, of weight S Re PROFILE_HT at X[i] inside the line's window;
 * out_f64[n_states][ld] and / or out_f32 = (float)(sum * scale). One workgroup per 256 points of a state; a point's bits
 * do not depend on the rest of the axis or on the other states.
 * rtx_ht_params: state `state` of the last prologue into DEVICE buffers (any may be NULL): params[n_lines][10] in
 * rtx_profile_eval's layout, strength[n_lines] = weight S (0: dropped), window[n_lines][2] = lo, hi.
 * Errors (before any device work): a required pointer NULL, a negative count, more states or points than the object was
 * created for, ld < n, a column set that does not exist, an axis that is not sorted. n_lines = 0 or nx = 0 succeeds without
 * a kernel launch (rtx_ht_sum on a table without lines writes zeros). Asynchronous on `stream` otherwise. */
#define RTX_HT_COLS 27
typedef struct rtx_ht rtx_ht;
int rtx_lines_set_ht(rtx_lines* lines, int n_sets, const int32_t* set_h, const double* const* cols_h);
int rtx_ht_create(int64_t n_lines, int max_states, int64_t max_points, rtx_ht** out);
int rtx_ht_free(rtx_ht* ht);
int rtx_ht_prep(rtx_ht* ht, const rtx_lines* lines, const double* X_h, int64_t nx, int n_states, const double* T_h,
                const double* p_atm_h, const double* qratio_h, const double* weight_h, const double* mass_h, int n_dil,
                const int32_t* dil_h, const double* frac_h, double omega_wing, double omega_wing_hw,
                double intensity_threshold, double scale, void* stream);
int rtx_ht_sum(const rtx_ht* ht, int n_states, float* out_f32, double* out_f64, int64_t ld, void* stream);
int rtx_ht_params(const rtx_ht* ht, int state, double* params, double* strength, int32_t* window, void* stream);

/* ---- post-processing of TUD products: smooth / reduceResolution ---------------------
 * Replaces radiative_transfer.py:1266-1324 (smooth: reflect-padded window convolution) and :1327-1350
 * (reduceResolution: symmetrised smoothing + scipy cubic interp1d onto a coarser axis).
 *   rtx_fir_reflect: out[r][i] = sum_k taps_h[k] * in[r][R(i + k - centre)], i in [0,n), fp64 accumulation;
 *       R reflects about the first and last sample (j<0 -> -j, j>=n -> 2(n-1)-j), the reference's padding (:1314).
 *       in: [n_rows][ld_in] float32 (in_is_f64 = 0) or float64 (1), device; taps_h: n_taps doubles on the HOST
 *       (n_taps <= 8192, n_taps - 1 <= n; with n_taps - 1 == n an index can need both reflections, -n -> n -> n - 2 and
 *       2n - 1 -> -1 -> 1: numpy.pad(mode="reflect"), period 2(n-1); n == 1: every index is sample 0);
 *       out: [n_rows][ld_out] float64, device.
 *   rtx_cubic_resample: the cubic spline through ALL samples of a uniform axis x0 + i*h, evaluated at x_out
 *       (device, fp64): in the interior scipy's not-a-knot interp1d(kind='cubic') is the cardinal cubic spline,
 *       whose coefficients are the samples filtered by sqrt(3)*(sqrt(3)-2)^|k|; truncated at |k| <= 40 (1e-23).
 *       Every x_out must lie in [x0 + 25 h, x0 + (n - 27) h] (error otherwise: the end conditions of the
 *       reference's spline, whose influence decays as 0.268^k, are not reproduced; at 25 knots it is 5e-15). Ysm: [n_rows][ld] float64; out: [n_rows][ld_out] float64. */
int rtx_fir_reflect(const void* in, int in_is_f64, int64_t ld_in, int n_rows, int64_t n,
                    const double* taps_h, int n_taps, int centre, double* out, int64_t ld_out,
                    void* stream);
int rtx_cubic_resample(const double* Ysm, int64_t ld, int n_rows, int64_t n, double x0, double h,
                       const double* x_out, int64_t n_out, double* out, int64_t ld_out, void* stream);
/* rtx_cubic_resample without its range check, which reads a flag back from the device and therefore synchronises the
 * stream: for a stream of spectra resampled onto ONE output axis that the caller has checked on the host (the loop of
 * Generate_LWIR_TUD.py:117-150 calls reduceResolution, radiative_transfer.py:1327-1350, once per atmosphere). Fully
 * asynchronous; an abscissa outside the supported range gives NaN. */
/* The end regions of the same spline (within a window length of either end of the axis the reference's knots are not
 * uniform -- it smooths the axis too, radiative_transfer.py:1331-1334, and smooth()'s reflection padding bends them -- and
 * the not-a-knot end condition acts): the not-a-knot spline on the m local samples Ysm[r][i_first .. i_first+m) with the TRUE
 * knots `knots[m]` (device, fp64; the smoothed axis there), natural at the cut; valid for x_out at least 24 knots inside
 * the cut (2e-14). high_end = 0: local sample 0 is the first sample of the axis; 1: local sample m-1 is the last one.
 * whole_axis = 1: the m samples are the whole (short) axis: not-a-knot at both ends, the reference's spline at every
 * x_out between the first and the last knot; 0: natural at the cut, as above. 4 <= m <= 768. out: [n_rows][ld_out]. */
int rtx_cubic_end(const double* Ysm, int64_t ld, int n_rows, int64_t i_first, int m, int high_end, int whole_axis,
                  const double* knots, const double* x_out, int64_t n_out, double* out, int64_t ld_out,
                  void* stream);
int rtx_cubic_resample_unchecked(const double* Ysm, int64_t ld, int n_rows, int64_t n, double x0, double h,
                                 const double* x_out, int64_t n_out, double* out, int64_t ld_out, void* stream);

/* ---- hapi's spectrum functions and slit-function convolution -------------------------------------------
 * rtx_hapi_spectrum replaces transmittanceSpectrum / absorptionSpectrum / radianceSpectrum, misc/hapi.py:11582-11680,
 * elementwise in fp64 and in the reference's order of operations:
 *   RTX_SPECTRUM_TRANSMITTANCE  exp(-k l)
 *   RTX_SPECTRUM_ABSORPTION     1 - exp(-k l)
 *   RTX_SPECTRUM_RADIANCE       (1 - exp(-k l)) * 2 hh cc^2 nu^3 / (exp(hh cc nu / (cBolts T)) - 1) * 1e-7, with hapi's own
 *                               constants hh, cc, cBolts (misc/hapi.py:84-86), W/sr/cm^2/cm^-1 (:11677)
 *   k [n_rows][ld] float32 (k_is_f64 = 0) or float64 (1): absorption coefficients, wavenumber-contiguous rows;
 *   l path length in cm, T in K (read for RADIANCE only); out [n_rows][ld_out] float64;
 *   wavenumbers (RADIANCE only): X[n] fp64 when X != NULL, else `grid` (grid->n == n). */
#define RTX_SPECTRUM_TRANSMITTANCE 0
#define RTX_SPECTRUM_ABSORPTION 1
#define RTX_SPECTRUM_RADIANCE 2
int rtx_hapi_spectrum(int kind, const rtx_grid* grid, const double* X, const void* k, int k_is_f64, int n_rows,
                      int64_t n, int64_t ld, double l, double T, double* out, int64_t ld_out, void* stream);
/* rtx_fir_same: a window of the zero-padded linear convolution, what numpy.convolve computes inside convolveSpectrum /
 * convolveSpectrumSame / convolveSpectrumFull (misc/hapi.py:11826-11900):
 *   out[r][o] = out_scale * sum_{k=0}^{m-1} taps_h[k] * in[r][first + o - k],  o in [0, n_out),  in[r][j] = 0 outside [0, n).
 * [first, first + n_out) must lie inside the n + m - 1 points of the full convolution: first = 0, n_out = n + m - 1 is
 * mode 'full'; first = (min(n,m) - 1) / 2 (integer division), n_out = max(n,m) is mode 'same' (checked
 * against NumPy for every n, m < 40; tests/test_spectra_host.py). in: [n_rows][ld_in] float32 (in_is_f64 = 0) or float64 (1), device; taps_h: m >= 1 doubles on the HOST;
 * out: [n_rows][ld_out] float64, device. fp64 throughout: a float32 sample is widened exactly, and every output is ONE
 * fma chain over k = 0 .. m-1 in ascending order, so results are bit-identical run to run and do not depend on n_rows,
 * on the window or on which other outputs are computed. A direct sum (no FFT). The device copy of a slit is cached by
 * content (16 slits per process): only the first call with a new slit allocates and synchronises.
 * Errors: m < 1, n < 1, n_rows < 1, a window outside the full convolution, a leading dimension smaller than its row.
 * rtx_fir_tile_points / rtx_fir_chunk_taps: outputs per workgroup and taps staged per pass (for tests at the edges). */
int rtx_fir_same(const void* in, int in_is_f64, int64_t ld_in, int n_rows, int64_t n, const double* taps_h,
                 int64_t m, double out_scale, int64_t first, int64_t n_out, double* out, int64_t ld_out,
                 void* stream);
int rtx_fir_tile_points(void);
int rtx_fir_chunk_taps(void);

/* ---- optical depths from AFIT_XS cross-section tables -----------------------------------
 * The reference writes one cross-section file per molecule and (T, p) state (misc/RT_gen_AbsXS_files.py:45-92) and has no
 * reader for them; this is the consumer. An rtx_xs_lut is the device copy of such a set: n_rows fp32 rows of nx points
 * on one uniform axis, x fastest, each row 16-byte aligned; which molecule and node a row belongs to, and the power of
 * two each molecule's rows were multiplied by, is the caller's book-keeping (radtxfr_amd/afit_xs.py: XsLut).
 *   rtx_xs_lut_create    n_mol molecules, n_rows rows in all, zero-filled. Allocates device memory and synchronises.
 *   rtx_xs_lut_free      waits for the device, then releases the table and its term buffers.
 *   rtx_xs_lut_bytes     device bytes of the table.
 *   rtx_xs_lut_set_rows  rows [row0, row0 + n_rows) <- rows_h[n_rows][nx] (host, dense), one hipMemcpy2DAsync on `stream`. From
 *                        page-locked memory the copy is asynchronous: the caller keeps rows_h unchanged until `stream` has
 *                        passed the copy. From pageable memory the call synchronises `stream`: the HIP runtime was
 *                        observed (ROCm 7.0, a copy of 8 KB) to return only once `stream` had reached the copy and the rows
 *                        had left rows_h, unlike its 1-D copies. That is the runtime's behaviour as observed, its reason
 *                        not looked into, and no promise of this library's: a caller who wants rows_h back at once waits
 *                        for `stream` itself.
 *   rtx_xs_lut_get_rows  the inverse, into rows_h; synchronises `stream`.
 *   rtx_xs_od            od_f32[l][i] = sum_{m < n_mol} sum_{c < 4} weight_h[l][m][c] * row rows_h[l][m][c] at point
 *                        x_offset + i, for l < n_layers, i < n: fp32 [n_layers][ld], the layout rtx_voigt_sum writes, so
 *                        rtx_tud takes it unchanged. rows_h / weight_h are HOST arrays [n_layers][n_mol][4] (the four
 *                        corners of the bracketing (T, p) cell, weights carrying column amount, bilinear factor and the
 *                        molecule's power of two); every row index is checked against the table, every weight must be
 *                        finite. Per point the sum is one fp32 fmaf chain in the order given (molecule, then corner); a
 *                        term whose weight is exactly 0 is skipped and its row is not read. The value of a point is thus a
 *                        function of (table, layer, point) alone: bit-identical for every x_offset / n cut of an axis.
 *                        The terms are copied (hipMemcpyAsync on `stream`, staged before returning) into a grow-only
 *                        device buffer owned by the table, one per stream that has used it: the first call on a stream,
 *                        or a larger one, allocates and therefore synchronises; every other call only enqueues.
 *                        16-byte accesses when x_offset and ld are multiples of 4 and od_f32 is 16-byte aligned
 *                        (point by point for the ragged end of the last tile); otherwise point by point throughout.
 *   rtx_xs_tile_points   consecutive points one workgroup owns (for tests at the edges).
 *   rtx_xs_od_d          the table's part of the columns rtx_tud_jacobian, rtx_tud_vjp and rtx_tud_jvp (and their _dod
 *                        forms) take, all of them in one pass over the table rows:
 *                          dOD_dT[l][i]  = sum_{m < n_mol} sum_{c < 4} weight_dT_h[l][m][c] * row rows_h[l][m][c]
 *                          K[s][l][i]    = sum_{c < 4} weight_K_h[s][l][c] * row rows_h[l][spec_mol_h[s]][c]
 *                        at point x_offset + i, for l < n_layers, i < n, s < n_spec: fp32 dOD_dT[n_layers][ld] and
 *                        K[n_spec][n_layers][ld]. The outputs are WRITTEN, as rtx_xs_od writes its own, not added to
 *                        (rtx_continuum_add_d then adds onto them). rows_h as for rtx_xs_od; weight_dT_h
 *                        [n_layers][n_mol][4] and weight_K_h [n_spec][n_layers][4] are HOST arrays of derivative weights
 *                        (radtxfr_amd/afit_xs.py: layer_terms_d); spec_mol_h[n_spec] names the table index of each
 *                        species' molecule: distinct values in [0, n_mol), n_spec <= 16. Either output may be NULL (with
 *                        its weights), not both; n_spec = 0 goes with K = NULL. Every row index is checked against the
 *                        table, every weight must be finite; n = 0 writes nothing. Each output value is one fp32 fmaf
 *                        chain from 0 in term order (molecule, then corner) over the terms whose weight FOR THAT OUTPUT
 *                        is not 0; a row both of whose weights are 0 is not read. A value is thus a function of (table,
 *                        layer, point) alone, bit-identical for every x_offset / n cut, and equal bit for bit to
 *                        rtx_xs_od run on the same fp32 weights (weight_dT_h; one molecule's weight_K_h, 0 elsewhere).
 *                        Staging as rtx_xs_od's (hipMemcpyAsync on `stream`, staged before returning) into a grow-only
 *                        device buffer of this entry's own in the table, one for each stream: the first call on a
 *                        stream, or a larger one, allocates; every other call only enqueues. 16-byte accesses when
 *                        x_offset and ld are multiples of 4 and dOD_dT and K are 16-byte aligned (point by point for the
 *                        ragged end of the last tile); otherwise point by point throughout. flags: none is defined,
 *                        pass 0. */
typedef struct rtx_xs_lut rtx_xs_lut;
int rtx_xs_lut_create(int n_mol, int64_t n_rows, int64_t nx, rtx_xs_lut** out);
int rtx_xs_lut_free(rtx_xs_lut* lut);
int64_t rtx_xs_lut_bytes(const rtx_xs_lut* lut);
int rtx_xs_lut_set_rows(rtx_xs_lut* lut, int64_t row0, int64_t n_rows, const float* rows_h, void* stream);
int rtx_xs_lut_get_rows(const rtx_xs_lut* lut, int64_t row0, int64_t n_rows, float* rows_h, void* stream);
int rtx_xs_od(rtx_xs_lut* lut, int64_t x_offset, int64_t n, int n_layers, const int32_t* rows_h, const float* weight_h,
              float* od_f32, int64_t ld, void* stream);
int rtx_xs_tile_points(void);
int rtx_xs_od_d(rtx_xs_lut* lut, int64_t x_offset, int64_t n, int n_layers, const int32_t* rows_h, const float* weight_dT_h,
                int n_spec, const int32_t* spec_mol_h, const float* weight_K_h, float* dOD_dT, float* K, int64_t ld, void* stream,
                unsigned flags);

/* ---- tabulated continuum absorption -------------------------------------------------------
 * LBLRTM, behind the reference's compute_OD, adds the collision-induced continua to its line sum (write_tape5 switches them
 * on, radiative_transfer.py:591-601). Here the user supplies the coefficient tables (radtxfr_amd/continuum.py) and
 *   rtx_continuum_add   od_f32[l][i] += R(nu_i, T_h[l]) * sum_{c < n_comp} max(0, sum_{k < 4} L_k(t) * A[c][l][j0 + k])
 * for l < n_layers and the grid's points i < grid->n, in place on fp32 [n_layers][ld] (the layout rtx_voigt_sum and
 * rtx_xs_od write, so rtx_tud takes it unchanged). nu_i is the grid value of the GLOBAL index grid->offset + i;
 * R = nu tanh(c2 nu / (2T)), c2 = 1.43877736830 cm K; component c has the uniform node axis v0_h[c] + j * dv_h[c],
 * j < n_nodes_h[c] (at least 4 nodes, dv > 0) and contributes where v0 <= nu <= v0 + (n - 1) dv (the sum formed unfused in
 * fp64), nothing elsewhere; j0 = clamp(floor((nu - v0) / dv) - 1, 0, n - 4), t = (nu - nu_j0) / dv formed in fp64 and then
 * rounded, L_k the cubic Lagrange basis on the nodes 0, 1, 2, 3. tables_h is a HOST array [n_comp][n_layers][ld_nodes]
 * of fp32 node values A (column amount, density scaling and coefficients folded in by the caller; every value of a
 * component's first n nodes must be finite, the columns after them are not read). The value added at a point is a
 * function of (tables, layer, global index) alone: bit-identical for every offset / n cut of an axis. T_h, the axes and the
 * tables are copied (hipMemcpyAsync on `stream`, staged before returning) into a grow-only device buffer the library keeps
 * for each (device, stream) that has called: the first call on a stream, or a larger one, allocates; every other call only
 * enqueues. 16-byte accesses when ld is a multiple of 4 and od_f32 is 16-byte aligned (point by point for the ragged end
 * of the last tile); otherwise point by point throughout. flags: none is defined, pass 0 (it follows the stream as in
 * rtx_tud_opts).
 *   rtx_continuum_tile_points   consecutive points one workgroup owns (for tests at the edges). */
int rtx_continuum_add(const rtx_grid* grid, int n_layers, const double* T_h, int n_comp, const double* v0_h,
                      const double* dv_h, const int32_t* n_nodes_h, const float* tables_h, int64_t ld_nodes, float* od_f32,
                      int64_t ld, void* stream, unsigned flags);
int rtx_continuum_tile_points(void);

/* ---- derivatives through the tabulated continuum -------------------------------------------
 * The continuum's part of the columns rtx_tud_jacobian, rtx_tud_vjp and rtx_tud_jvp (and their _dod forms) take. With
 * s_c = sum_{k < 4} L_k(t) * A[c][l][j0 + k] the stencil sum rtx_continuum_add clamps, m_c = [s_c > 0], and s_T,c / s_x,c
 * the same stencil and weights on the node rows dA/dT (per K) and dA/dMF (per ppmv of the component's own molecule),
 *   rtx_continuum_add_d   dOD_dT[l][i]        += R_T * sum_c max(0, s_c) + R * sum_c m_c * s_T,c
 *                         K[slot_h[c]][l][i]  += R * m_c * s_x,c      for every component with slot_h[c] >= 0
 * for l < n_layers and the grid's points i < grid->n, in place on fp32 dOD_dT[n_layers][ld] and K[n_spec][n_layers][ld];
 * R as in rtx_continuum_add, R_T = dR/dT = -nu (c2 nu / (2 T^2)) sech^2(c2 nu / (2 T)). The grid, T_h, the axes and
 * tables_h are those of rtx_continuum_add (the same stencils, weights and fp32 operations: m_c is set exactly where that
 * call added something; where s_c <= 0, and outside a component's axis, both derivatives are 0: the kink of max(0, .) is
 * given the value 0). tables_dT_h and tables_dx_h are HOST arrays laid out as tables_h, finite on every component's nodes.
 * slot_h[n_comp] names the K slot of each component's molecule, -1 for a molecule that is not differentiated; several
 * components may share a slot, every slot lies in [-1, n_spec). dOD_dT may be NULL (no temperature term; tables_dT_h is
 * then not read and may be NULL), K may be NULL when every slot is -1 (tables_dx_h is then not read and may be NULL), not
 * both. Each destination row is read and written once per group of four components, the group's terms summed first: on
 * a block of zeros the result is the derivative itself, on any block `block + that` rounded once (for up to four
 * components). The value added at a point is a function of (tables, layer, global index) alone: bit-identical for every
 * offset / n cut of an axis. Staging (hipMemcpyAsync on `stream`, staged before returning, into a grow-only device buffer
 * of this entry's own per (device, stream)) and the 16-byte accesses (ld a multiple of 4, dOD_dT and K 16-byte aligned)
 * as in rtx_continuum_add. flags: none is defined, pass 0. */
int rtx_continuum_add_d(const rtx_grid* grid, int n_layers, const double* T_h, int n_comp, const double* v0_h,
                        const double* dv_h, const int32_t* n_nodes_h, const float* tables_h, const float* tables_dT_h,
                        const float* tables_dx_h, int64_t ld_nodes, const int32_t* slot_h, int n_spec, float* dOD_dT, float* K,
                        int64_t ld, void* stream, unsigned flags);

/* ------------------------------------------------------------------------------------------
 * Single-process collectives over the GPUs of one node. The reference has no multi-GPU code; its scripts are plain
 * Python programs that fan work out with multiprocessing (Generate_LWIR_TUD.py:117-150). These three calls let ONE host
 * process shard a spectrum over several devices and reassemble it -- the one exchange of the path: the all-gather of the
 * packed [tau, L-up, L-down] blocks (radtxfr_amd/dist.py: compute_TUD_local) -- without a launcher.
 *   rtx_comm_init_all  devs_h[ndev] device indices. backend -1: RCCL (ncclCommInitAll, resolved at run time from the
 *                      librccl the process already holds, else librccl.so) when it loads and the devices are distinct,
 *                      otherwise peer copies; 0: peer copies (hipMemcpyPeerAsync fan-out; a device may repeat); 1: RCCL or
 *                      fail. Environment RADTXFR_COMM=peer|rccl overrides. Allocates and synchronises.
 *   rtx_comm_backend   0 peer copies, 1 RCCL
 *   rtx_allgather      rank i contributes sendbufs_h[i][0..count) float32 on device devs[i]; afterwards every
 *                      recvbufs_h[j][i*count + t] = sendbufs_h[i][t]. streams_h[i] is rank i's stream (send block complete
 *                      in its order before, gathered block complete in its order after). Asynchronous to the host. */
typedef struct rtx_comm rtx_comm;
int rtx_comm_init_all(int ndev, const int* devs_h, int backend, rtx_comm** out);
int rtx_comm_backend(const rtx_comm* comm);
int rtx_allgather(rtx_comm* comm, const void* const* sendbufs_h, void* const* recvbufs_h, int64_t count,
                  void* const* streams_h);
int rtx_comm_destroy(rtx_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* RADTXFR_HIP_H */
