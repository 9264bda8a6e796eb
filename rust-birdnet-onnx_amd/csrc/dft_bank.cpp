// Recognition of a filter bank as a windowed DFT from its weights, and the two launches such a bank can become.  See dft_bank.h.
#include "dft_bank.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#include "plan_rules.h"

namespace bn {

static void host_fft(std::vector<double> &re, std::vector<double> &im) {  // in-place radix-2, n a power of two
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; i++) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * M_PI / (double)len;
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; k++) {
                const double wr = std::cos(ang * (double)k), wi = std::sin(ang * (double)k);
                const size_t u = i + k, v = i + k + len / 2;
                const double xr = re[v] * wr - im[v] * wi, xi = re[v] * wi + im[v] * wr;
                re[v] = re[u] - xr; im[v] = im[u] - xi;
                re[u] += xr; im[u] += xi;
            }
    }
}
// L = 10 * 4^j * 16 ... in the kernel's terms: M = L / 2 = 5 q with q = 4^j * 16 a power of FOUR times 16 (radix 5 first, then
// radix-4 passes down to the 16-point register blocks; a radix-2 pass exists only as a FIRST pass) -- 640 is the one in use
bool fft_five_pow2(int64_t L) {
    if (L % 10) return false;
    int64_t q = L / 10;
    if (q < 64 || (q & (q - 1))) return false;
    int lg = 0;
    while (((int64_t)1 << lg) < q) lg++;
    return lg % 2 == 0;  // q = 16 * 4^j
}
// bins 0 .. n/2 of the DFT of a real row by the definition (any n; the peak search below reads no other bin)
static void host_dft_half(std::vector<double> &re, std::vector<double> &im) {
    const size_t n = re.size();
    std::vector<double> c(n), s_(n), xr(re);
    for (size_t t = 0; t < n; t++) { c[t] = std::cos(2.0 * M_PI * (double)t / (double)n); s_[t] = std::sin(2.0 * M_PI * (double)t / (double)n); }
    for (size_t k = 0; k <= n / 2; k++) {
        double ar = 0, ai = 0;
        for (size_t t = 0; t < n; t++) {
            const size_t ph = (k * t) % n;
            ar += xr[t] * c[ph];
            ai -= xr[t] * s_[ph];
        }
        re[k] = ar; im[k] = ai;
    }
}
bool detect_dft_bank(const std::vector<float> &wf, int64_t Cout, int64_t L, const std::vector<int> &cls, DftBank &bank) {
    const bool pow2 = (L & (L - 1)) == 0;
    if (L < 128 || L > 2048 || !(pow2 || fft_five_pow2(L))) return false;
    const double tol = sw_double(sw::BN_STFT_TOL);
    bank.L = L;
    bank.k.assign((size_t)Cout, 0);
    bank.a.assign((size_t)Cout, 0.0);
    bank.b.assign((size_t)Cout, 0.0);
    std::vector<double> rowmax((size_t)Cout, 0.0);
    std::vector<char> is_sin((size_t)Cout, 0), live((size_t)Cout, 0);
    double gmax = 0;
    for (float v : wf) gmax = std::max(gmax, (double)std::fabs(v));
    for (int64_t c = 0; c < Cout; c++) {
        const float *w = &wf[(size_t)(c * L)];
        double mx = 0;
        for (int64_t n = 0; n < L; n++) mx = std::max(mx, (double)std::fabs(w[n]));
        rowmax[(size_t)c] = mx;
        // a row whose largest tap is below f32 resolution of the bank's largest tap (sin(pi n) of the Nyquist bin
        // evaluated in floating point: ~1e-13) counts as the zero row it stands for
        if (!(mx > 1e-7 * gmax)) continue;
        live[(size_t)c] = 1;
        is_sin[(size_t)c] = cls[(size_t)c] < 0;
        std::vector<double> re(w, w + L), im((size_t)L, 0.0);
        if (pow2) host_fft(re, im);
        else host_dft_half(re, im);
        int best = 0;
        double bm = -1;
        for (int64_t q = 0; q <= L / 2; q++) {
            const double m2 = re[(size_t)q] * re[(size_t)q] + im[(size_t)q] * im[(size_t)q];
            if (m2 > bm) { bm = m2; best = (int)q; }
        }
        bank.k[(size_t)c] = best;
    }
    // unit sinusoids of every live row, from one table of cos(2 pi t / L)
    std::vector<double> ctab((size_t)L);
    for (int64_t t = 0; t < L; t++) ctab[(size_t)t] = std::cos(2.0 * M_PI * (double)t / (double)L);
    auto trig = [&](int64_t c, int64_t n) {
        const int64_t ph = ((int64_t)bank.k[(size_t)c] * n) % L;  // exact phase reduction
        return is_sin[(size_t)c] ? ctab[(size_t)((ph + 3 * L / 4) % L)] : ctab[(size_t)ph];  // sin x = cos(x - pi/2)
    };
    std::vector<double> amp((size_t)Cout, 0.0), win((size_t)L, 0.0), energy((size_t)Cout, 0.0);
    for (int64_t c = 0; c < Cout; c++) {
        if (!live[(size_t)c]) continue;
        double e = 0;
        for (int64_t n = 0; n < L; n++) e += (double)wf[(size_t)(c * L + n)] * wf[(size_t)(c * L + n)];
        energy[(size_t)c] = e;
    }
    // start from the row energy: sum (w t)^2 is ~ sum w^2 / 2 for a sinusoid, sum w^2 for the DC / Nyquist rows
    // (the sign settles in the first amplitude step)
    auto init_amp = [&](int64_t c) {
        const int k = bank.k[(size_t)c];
        amp[(size_t)c] = std::sqrt(energy[(size_t)c] * ((k == 0 || k == L / 2) ? 1.0 : 2.0));
    };
    std::vector<char> use((size_t)Cout, 0);
    auto als = [&](int max_it) {
        for (int it = 0; it < max_it; it++) {
            for (int64_t n = 0; n < L; n++) {
                double num = 0, den = 0;
                for (int64_t c = 0; c < Cout; c++) {
                    if (!use[(size_t)c]) continue;
                    const double t = amp[(size_t)c] * trig(c, n);
                    num += t * (double)wf[(size_t)(c * L + n)];
                    den += t * t;
                }
                win[(size_t)n] = den > 0 ? num / den : 0.0;
            }
            double wmax = 0;
            for (double v : win) wmax = std::max(wmax, std::fabs(v));
            if (!(wmax > 0)) return false;
            for (double &v : win) v /= wmax;
            double change = 0;
            for (int64_t c = 0; c < Cout; c++) {
                if (!use[(size_t)c]) continue;
                double num = 0, den = 0;
                for (int64_t n = 0; n < L; n++) {
                    const double t = win[(size_t)n] * trig(c, n);
                    num += t * (double)wf[(size_t)(c * L + n)];
                    den += t * t;
                }
                if (!(den > 0)) return false;  // e.g. a sine row at bin 0: identically zero model, non-zero row
                const double na = num / den;
                change = std::max(change, std::fabs(na - amp[(size_t)c]) / std::max(std::fabs(na), 1e-300));
                amp[(size_t)c] = na;
            }
            if (it > 0 && change < 1e-11) break;
        }
        return true;
    };
    // stage 1: rows whose spectral peak is unambiguous (bins 3 .. L/2 - 3: near DC and Nyquist the two mirror
    // lobes of a windowed sinusoid overlap and the peak can sit one bin off) give a first window estimate
    int64_t n_sure = 0;
    for (int64_t c = 0; c < Cout; c++) {
        use[(size_t)c] = live[(size_t)c] && bank.k[(size_t)c] >= 3 && bank.k[(size_t)c] <= L / 2 - 3;
        n_sure += use[(size_t)c];
        if (live[(size_t)c]) init_amp(c);
    }
    if (n_sure == 0)
        for (int64_t c = 0; c < Cout; c++) use[(size_t)c] = live[(size_t)c];
    // The amplitude SIGNS are unknown at this point (exporters write -sin rows next to +cos rows: with all-positive
    // starting amplitudes the cos^2 and sin^2 contributions to a least-squares window cancel), so the first window
    // comes from energies, which do not see signs: sum_c R_c[n]^2 = w[n]^2 sum_c a_c^2 t_c[n]^2, w >= 0 as every
    // analysis window in use is.  The first amplitude step then settles the signs.
    {
        double wmax = 0;
        for (int64_t n = 0; n < L; n++) {
            double num = 0, den = 0;
            for (int64_t c = 0; c < Cout; c++) {
                if (!use[(size_t)c]) continue;
                const double t = amp[(size_t)c] * trig(c, n), r = (double)wf[(size_t)(c * L + n)];
                num += r * r;
                den += t * t;
            }
            win[(size_t)n] = den > 0 ? std::sqrt(num / den) : 0.0;
            wmax = std::max(wmax, win[(size_t)n]);
        }
        if (!(wmax > 0)) return false;
        for (double &v : win) v /= wmax;
        for (int64_t c = 0; c < Cout; c++) {
            if (!use[(size_t)c]) continue;
            double num = 0, den = 0;
            for (int64_t n = 0; n < L; n++) {
                const double t = win[(size_t)n] * trig(c, n);
                num += t * (double)wf[(size_t)(c * L + n)];
                den += t * t;
            }
            if (!(den > 0)) return false;
            amp[(size_t)c] = num / den;
        }
    }
    if (!als(3)) return false;
    // stage 2: every row's bin re-decided among the neighbours of its peak by the least-squares residual against
    // that window
    for (int64_t c = 0; c < Cout; c++) {
        if (!live[(size_t)c]) continue;
        const int k0 = bank.k[(size_t)c];
        int best = k0;
        double best_res = INFINITY;
        for (int k = std::max(0, k0 - 2); k <= std::min<int>((int)(L / 2), k0 + 2); k++) {
            bank.k[(size_t)c] = k;
            double num = 0, den = 0;
            for (int64_t n = 0; n < L; n++) {
                const double t = win[(size_t)n] * trig(c, n);
                num += t * (double)wf[(size_t)(c * L + n)];
                den += t * t;
            }
            const double res = den > 0 ? energy[(size_t)c] - num * num / den : INFINITY;
            if (res < best_res) { best_res = res; best = k; }
        }
        if (sw_present(sw::BN_STFT_DEBUG) && (c < 4 || best != k0))
            fprintf(stderr, "stft: row %lld %s peak bin %d -> %d (residual %.3g of energy %.3g)\n", (long long)c, is_sin[(size_t)c] ? "sin" : "cos", k0, best,
                    best_res, energy[(size_t)c]);
        bank.k[(size_t)c] = best;
        {  // amplitude (with its sign) against the stage-1 window
            double num = 0, den = 0;
            for (int64_t n = 0; n < L; n++) {
                const double t = win[(size_t)n] * trig(c, n);
                num += t * (double)wf[(size_t)(c * L + n)];
                den += t * t;
            }
            if (!(den > 0)) return false;
            amp[(size_t)c] = num / den;
        }
        use[(size_t)c] = 1;
    }
    // stage 3: all rows
    if (!als(40)) return false;
    // the window in f32 (what the kernel multiplies by); amplitudes refitted against the rounded window, then verify
    bank.window.resize((size_t)L);
    for (int64_t n = 0; n < L; n++) bank.window[(size_t)n] = (float)win[(size_t)n];
    for (int64_t c = 0; c < Cout; c++) {
        if (!live[(size_t)c]) continue;
        for (int64_t n = 0; n < L; n++) {
            const double model = amp[(size_t)c] * win[(size_t)n] * trig(c, n);
            if (!(std::fabs(model - (double)wf[(size_t)(c * L + n)]) <= tol * rowmax[(size_t)c])) {
                if (sw_present(sw::BN_STFT_DEBUG))
                    fprintf(stderr, "stft: row %lld (bin %d, %s) tap %lld: model %.9g vs %.9g (row max %.3g)\n", (long long)c, bank.k[(size_t)c],
                            is_sin[(size_t)c] ? "sin" : "cos", (long long)n, model, (double)wf[(size_t)(c * L + n)], rowmax[(size_t)c]);
                return false;
            }
        }
        if (is_sin[(size_t)c]) bank.b[(size_t)c] = amp[(size_t)c];
        else bank.a[(size_t)c] = amp[(size_t)c];
    }
    return true;
}
// digit-reversed position of output k of an in-place DIF transform with the given radix sequence
static int dif_position(int k, int n, const std::vector<int> &radix, size_t idx) {
    if (n == 1) return 0;
    const int r = radix[idx];
    return (k % r) * (n / r) + dif_position(k / r, n / r, radix, idx + 1);
}
bool emit_stft(Plan &plan, const std::string &name, const PlanOp &base, const DftBank &bank, int64_t Cout, int64_t OW, bool has_bias) {
    // Which banks run as FFTs.  The alternative is the pruned + folded matrix product on the exact-f32 MFMA path, whose
    // cost follows the number of LIVE bins: Cout * L/2 multiply-adds at 32 per SIMD-cycle, against roughly
    // 0.18 * L * log2 L cycles of vector butterflies, address arithmetic and LDS traffic for the FFT plus its untangle
    // and mel phases (both calibrated on the v2.4 banks, DESIGN.md section 4.11: L = 2048 with 127 live bins -- matrix
    // product 69 us, FFT 76-93 us; L = 1024 with 309 live bins -- 85 us vs 62-75 us).  Default ("auto"): FFT when the
    // matrix product is estimated at more than 1.5x the FFT.  BN_STFT=1: every recognised bank; BN_STFT=0: none;
    // BN_STFT_MINBINS=<n> additionally keeps banks with fewer live bins on the matrix path.
    if (sw_is(sw::BN_STFT, "0")) return false;
    if (Cout < sw_i64(sw::BN_STFT_MINBINS)) return false;
    if (!sw_is(sw::BN_STFT, "1")) {
        const double lg = std::log2((double)bank.L);
        const double gemm_cycles = (double)Cout * (double)(bank.L / 2) / 32.0, fft_cycles = 0.18 * (double)bank.L * lg;
        if (!(gemm_cycles > 1.5 * fft_cycles)) return false;
    }
    const GemmDesc &g = base.gemm;
    if (g.act != ACT_NONE || g.has_res || g.has_scale || g.lda <= 0 || g.lda > 4096 || g.ldc != Cout) return false;
    const int L = (int)bank.L, M = L / 2;
    PlanOp op;
    op.kind = OpKind::FFT;
    op.name = "stft:" + name;
    op.r.out = base.r.out;
    op.r.a = base.r.a;
    op.r.bias = base.r.bias;
    FftDesc &d = op.fft;
    d.L = L; d.M = M; d.hop = (int32_t)g.lda; d.frames = (int32_t)OW; d.nout = (int32_t)Cout;
    d.logM = 0;
    while ((1 << d.logM) < M) d.logM++;
    d.F = 1024 / M;
    const bool five = M % 5 == 0;  // M = 5 q (detect_dft_bank: q = 16 * 4^j): three frames of 320 slots per wave pass
    // frames per tile: as many as keep the tile's signal span within the kernel's staging registers (8192 floats)
    if (five) {
        // whole wave passes, one per wave of the block where the span allows: 8 waves x F frames
        d.tpb = 8 * d.F;
        while (d.tpb > d.F && (int64_t)(d.tpb - 1) * g.lda + L > 8192) d.tpb -= d.F;
    } else {
        d.tpb = 16;
        while (d.tpb > d.F && (int64_t)(d.tpb - 1) * g.lda + L > 8192) d.tpb /= 2;
    }
    if ((int64_t)(d.tpb - 1) * g.lda + L > 8192 || d.tpb % d.F) return false;
    d.a_bs = g.a_bs; d.ldc = g.ldc; d.c_bs = g.c_bs; d.has_bias = has_bias ? 1 : 0;
    d.out_rs = g.ldc; d.out_cs = 1;
    d.power = 0; d.otab_stride = 8;
    // pass structure: radix 5 first for M = 5 q, radix 2 first when log2 M is odd, radix 4 down to 16-point blocks (registers)
    std::vector<int> radix;
    std::vector<float> tw;
    int nn = M;
    d.npass = 0;
    while (nn > 16) {
        const int r = (d.npass == 0 && five) ? 5 : (d.npass == 0 && (d.logM & 1)) ? 2 : 4;
        if (nn % r) return false;
        const int q = nn / r;
        d.pass_n[d.npass] = nn; d.pass_r[d.npass] = r; d.pass_tw[d.npass] = (int32_t)(tw.size() / 2);
        for (int pw = 1; pw < r; pw++)
            for (int j = 0; j < q; j++) {
                const double ang = -2.0 * M_PI * (double)((int64_t)j * pw % nn) / (double)nn;
                tw.push_back((float)std::cos(ang));
                tw.push_back((float)std::sin(ang));
            }
        radix.push_back(r);
        nn = q;
        d.npass++;
    }
    if (nn != 16 || d.npass > 4) return false;
    radix.push_back(4);
    radix.push_back(4);
    d.tw_count = (int32_t)(tw.size() / 2);
    if (stft_lds_bytes(d, 8) > 156 * 1024) return false;
    // per-output table
    std::vector<float> otab((size_t)Cout * 8, 0.0f);  // per output: positions of Z[k], Z[M-k] (as floats), 4 coefficients, 2 pad
    auto physpos = [&](int k) {
        const int pp = dif_position(k, M, radix, 0);
        return pp + 2 * (pp >> 4);
    };
    for (int64_t c = 0; c < Cout; c++) {
        const int k = bank.k[(size_t)c];
        const double a = bank.a[(size_t)c], b = bank.b[(size_t)c];
        const double th = 2.0 * M_PI * (double)k / (double)L, cs = std::cos(th), sn = std::sin(th);
        float *e = &otab[(size_t)c * 8];
        e[0] = (float)physpos(k % M);
        e[1] = (float)physpos((M - k % M) % M);
        e[2] = (float)(0.5 * (a * (1.0 - sn) + b * cs));
        e[3] = (float)(0.5 * (a * cs - b * (1.0 - sn)));
        e[4] = (float)(0.5 * (a * (1.0 + sn) - b * cs));
        e[5] = (float)(0.5 * (a * cs + b * (1.0 + sn)));
    }
    op.r.fft.window = Ref{Space::CONSTS, add_const(plan, bank.window), 0};
    op.r.fft.twiddles = Ref{Space::CONSTS, add_const(plan, tw), 0};
    op.r.fft.otab = Ref{Space::CONSTS, add_const(plan, otab), 0};
    const double log2L = std::log2((double)L);
    op.flops_fft = (double)OW * 2.5 * L * log2L;
    op.macs = op.flops_fft / 2;  // multiply-add equivalents actually performed (vector ALU)
    op.mfma = false;
    op.weight_bytes = 4.0 * (bank.window.size() + tw.size() + otab.size() + (has_bias ? Cout : 0));
    op.bytes = base.bytes;
    plan.dft_gemm_macs += (double)OW * Cout * L;  // what the matrix-product evaluation of this bank multiplies
    plan.dft_fft_equiv_flops += op.flops_fft;
    plan.dft_performed_macs += op.flops_fft / 2;
    push_op(plan, std::move(op));
    return true;
}

// ------------------------------------------------------------- quarter-folded cosine banks (round 4)
// A recognised bank of windowed COSINES only (the real part of an STFT) with a window symmetric about the frame centre: the even
// bins see the frame through S[n] = ye[n] + ye[L/2 - n], the odd ones through D[n] = ye[n] - ye[L/2 - n], n <= L/4 (kernels.h,
// GemmDesc::fold == 2; kernels.hip, frame_fold2_kernel) -- L/4 + 1 taps per output instead of L/2.  The filter rows become pure
// cosines x the fitted row amplitude (double -> f32), the window moves to the signal (two tables), the columns are grouped (even bins,
// padded to 32, then odd bins) and a column map sends every result to its output channel.  v2.4's 127 mel-live bins of the 2048-point
// branch: 17 K steps instead of 32.  BN_CONVFOLD2=0 keeps the half fold.
bool emit_quarter_fold(Plan &plan, const std::string &name, const PlanOp &base, const DftBank &bank, const std::vector<int> &cls, int64_t Cout, int64_t OW, bool has_bias) {
    if (sw_int(sw::BN_CONVFOLD2) == 0) return false;
    const int64_t L = bank.L;
    if (L % 128 != 0) return false;
    for (int64_t c = 0; c < Cout; c++)
        if (cls[(size_t)c] < 0 || bank.b[(size_t)c] != 0.0) return false;  // a sine row: the half fold (or the FFT) keeps the bank
    // the window: symmetric about the centre, nothing at tap 0 (the fold check saw that on the rows; here on the fitted window itself)
    // (a tap at which every row's cosine vanishes -- n = L/4 for a bank of odd bins -- is invisible in the rows: the fitted window holds
    // noise there, and nothing it multiplies reaches an output.  Such taps count as zero.)
    std::vector<float> w = bank.window;
    {
        std::vector<double> seen((size_t)L, 0.0);
        double smax = 0;
        for (int64_t t = 0; t < L; t++) {
            for (int64_t c = 0; c < Cout; c++) {
                const double v = bank.a[(size_t)c] * std::cos(2.0 * M_PI * (double)((bank.k[(size_t)c] * t) % L) / (double)L);
                seen[(size_t)t] += v * v;
            }
            smax = std::max(smax, seen[(size_t)t]);
        }
        for (int64_t t = 0; t < L; t++)
            if (!(seen[(size_t)t] > 1e-20 * smax)) w[(size_t)t] = 0.0f;
    }
    float wmax = 0.0f;
    for (float v : w) wmax = std::max(wmax, std::fabs(v));
    const float eps = 4e-7f * wmax;
    const bool dbg = sw_present(sw::BN_STFT_DEBUG);
    if (!(std::fabs(w[0]) <= eps)) {
        if (dbg) fprintf(stderr, "quarter fold: window tap 0 = %.3g\n", (double)w[0]);
        return false;
    }
    for (int64_t t = 1; t < L / 2; t++)
        if (!(std::fabs(w[(size_t)t] - w[(size_t)(L - t)]) <= eps)) {
            if (dbg) fprintf(stderr, "quarter fold: window not symmetric at tap %lld: %.9g vs %.9g\n", (long long)t, (double)w[(size_t)t], (double)w[(size_t)(L - t)]);
            return false;
        }
    std::vector<int32_t> even, odd, dead;
    for (int64_t c = 0; c < Cout; c++) (bank.a[(size_t)c] == 0.0 ? dead : (bank.k[(size_t)c] & 1) ? odd : even).push_back((int32_t)c);
    for (int32_t c : dead) {  // an all-zero row (its output is the bias) joins the group with room in its last wave column
        const size_t se = (32 - even.size() % 32) % 32, so = (32 - odd.size() % 32) % 32;
        (so > se ? odd : even).push_back(c);
    }
    const int64_t ne = ((int64_t)even.size() + 31) / 32 * 32, no = ((int64_t)odd.size() + 31) / 32 * 32, N2 = ne + no;
    const int64_t Q = L / 4, K2 = Q + 32;
    PlanOp f = base;
    f.gemm.N = (int32_t)N2;
    f.gemm.K = (int32_t)K2;
    f.gemm.fold = 2;
    f.gemm.fold_n = (int32_t)L;
    f.gemm.fold_ne = (int32_t)ne;
    if (!frame_fold2_shape_ok(f.gemm, nullptr)) {
        if (dbg) fprintf(stderr, "quarter fold: shape outside the kernel (N = %lld + %lld columns, %zu bytes of LDS)\n", (long long)ne, (long long)no, frame_fold2_lds_bytes(f.gemm));
        return false;
    }
    std::vector<float> colmap_bits((size_t)N2), wk((size_t)(N2 * K2), 0.0f), tabs((size_t)(2 * K2), 0.0f);
    std::vector<int32_t> colmap((size_t)N2, -1);
    for (size_t i = 0; i < even.size(); i++) colmap[i] = even[i];
    for (size_t i = 0; i < odd.size(); i++) colmap[(size_t)ne + i] = odd[i];
    static_assert(sizeof(int32_t) == sizeof(float), "the column map travels in a constant of floats");
    std::memcpy(colmap_bits.data(), colmap.data(), (size_t)N2 * sizeof(float));
    std::vector<double> ctab((size_t)L);
    for (int64_t t = 0; t < L; t++) ctab[(size_t)t] = std::cos(2.0 * M_PI * (double)t / (double)L);
    for (int64_t col = 0; col < N2; col++) {
        const int32_t c = colmap[(size_t)col];
        if (c < 0) continue;
        const int64_t k = bank.k[(size_t)c];
        const double a = bank.a[(size_t)c];
        float *row = &wk[(size_t)(col * K2)];
        for (int64_t t = 0; t < Q; t++) row[t] = (float)(a * ctab[(size_t)((k * t) % L)]);
        row[Q] = (k & 1) ? 0.0f : (float)(a * ctab[(size_t)((k * Q) % L)]);  // cos(pi k / 2) = +-1 for even k
    }
    // S[n] = wa[n] (x[n] + x[L-n]) + wb[n] (x[L/2-n] + x[L/2+n]); n = 0: ye[0] = 0 and ye[L/2] = y[L/2] once; n = L/4: ye[L/4] once
    for (int64_t t = 1; t < Q; t++) {
        tabs[(size_t)t] = w[(size_t)t];
        tabs[(size_t)(K2 + t)] = w[(size_t)(L / 2 - t)];
    }
    tabs[0] = 0.0f;
    tabs[(size_t)K2] = 0.5f * w[(size_t)(L / 2)];
    tabs[(size_t)Q] = w[(size_t)Q];
    tabs[(size_t)(K2 + Q)] = 0.0f;
    f.name = "Conv:" + name + "~quarter";
    if (frame_fold2q_ok(f.gemm)) {  // (round 5) half-height blocks on the bf16 matrix pipe: three exact bf16 planes per filter element, fragment order
        const int64_t steps = K2 / 32;
        std::vector<uint16_t> img((size_t)(N2 * K2 * 3), 0);  // [column group][step][16-wide k group][plane][lane][8]
        for (int64_t wn = 0; wn < N2 / 32; wn++)
            for (int64_t ks = 0; ks < steps; ks++)
                for (int64_t g = 0; g < 2; g++)
                    for (int64_t lane = 0; lane < 64; lane++) {
                        const int64_t lr = lane & 31, lh = lane >> 5;
                        for (int64_t j = 0; j < 8; j++) {
                            uint16_t h, m, l;
                            split_bf16x3(wk[(size_t)((wn * 32 + lr) * K2 + ks * 32 + 16 * g + 8 * lh + j)], h, m, l);
                            const size_t at = (size_t)(((((wn * steps + ks) * 2 + g) * 3) * 64 + lane) * 8 + j);
                            img[at] = h;
                            img[at + 64 * 8] = m;
                            img[at + 2 * 64 * 8] = l;
                        }
                    }
        std::vector<float> pk(img.size() / 2);
        std::memcpy(pk.data(), img.data(), img.size() * sizeof(uint16_t));
        wk.swap(pk);
        f.gemm.fold_wpk = 2;
    } else if (frame_fold2p_ok(f.gemm)) {  // half-height blocks: the filter fragments in the order the waves load them
        const int64_t steps = K2 / 32;
        std::vector<float> pk((size_t)(N2 * K2));
        for (int64_t wn = 0; wn < N2 / 32; wn++)
            for (int64_t ks = 0; ks < steps; ks++)
                for (int64_t g = 0; g < 4; g++)
                    for (int64_t lane = 0; lane < 64; lane++) {
                        const int64_t lr = lane & 31, lh = lane >> 5;
                        for (int64_t j = 0; j < 4; j++)
                            pk[(size_t)((((wn * steps + ks) * 4 + g) * 64 + lane) * 4 + j)] = wk[(size_t)((wn * 32 + lr) * K2 + ks * 32 + 8 * g + 4 * lh + j)];
                    }
        wk.swap(pk);
        f.gemm.fold_wpk = 1;
    }
    f.r.w = Ref{Space::CONSTS, add_const(plan, wk), 0};
    f.r.fold2.tables = Ref{Space::CONSTS, add_const(plan, tabs), 0};
    f.r.fold2.colmap = Ref{Space::CONSTS, add_const(plan, colmap_bits), 0};
    f.macs = (double)OW * (double)Cout * (double)(Q + 1);  // multiplications actually performed (padding columns excluded)
    f.weight_bytes = 4.0 * (wk.size() + tabs.size() + colmap.size() + (has_bias ? Cout : 0));
    plan.dft_gemm_macs += (double)OW * Cout * L;
    plan.dft_performed_macs += f.macs;
    plan.dft_fft_equiv_flops += (double)OW * 2.5 * (double)L * std::log2((double)L);
    push_op(plan, std::move(f));
    return true;
}

}  // namespace bn
