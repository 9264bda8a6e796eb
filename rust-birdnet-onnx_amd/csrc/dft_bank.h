// A filter bank recognised as a windowed DFT, and the launches it becomes (dft_bank.cpp; private to the planner, see plan_build.h).
#pragma once
#include "plan_build.h"

namespace bn {
#pragma GCC visibility push(hidden)

// ------------------------------------------------------------- windowed-DFT filter banks -> real FFT
// A single-channel 1-D filter bank whose every row is  a_c * w[n] * cos(2 pi k_c n / L)  (symmetric rows) or
// b_c * w[n] * sin(2 pi k_c n / L)  (antisymmetric rows) for ONE common window w and integer bins k_c is a
// short-time Fourier transform: out[c] = a_c Re Y[k_c] - b_c Im Y[k_c] with Y = FFT(w . frame).  The bank is
// recognised from the numbers alone (the exporter's node names say nothing): bins by the peak of each row's
// spectrum, window and amplitudes by alternating least squares over all rows, and the model is accepted only if
// every tap of every row agrees with it within f32 rounding of the taps (BN_STFT_TOL x max|row|, default 4e-7).
// Then ONE launch of stft_kernel (kernels.h, FftDesc) computes all rows -- cos and sin blocks together -- instead
// of one folded GEMM per symmetry run.  L must be a power of two in 128..2048, or five times a power of two (Perch's L = 640:
// mixed radix 5 x 4 x 16).  Whether a recognised bank runs as an FFT: emit_stft.
struct DftBank {
    int64_t L = 0;
    std::vector<float> window;
    std::vector<int> k;
    std::vector<double> a, b;
};

// lengths the FFT kernel takes besides the powers of two: L = 10 q, q = 16 * 4^j (640)
bool fft_five_pow2(int64_t L);
// cls[c]: +1 symmetric row, -1 antisymmetric, 0 all-zero (fold_framing_conv's classification); false: not a windowed-DFT bank
bool detect_dft_bank(const std::vector<float> &wf, int64_t Cout, int64_t L, const std::vector<int> &cls, DftBank &bank);
// `base`: the framing GEMM the bank would otherwise be; `name`: its node's.  true: the launch was pushed; false: nothing was
bool emit_stft(Plan &plan, const std::string &name, const PlanOp &base, const DftBank &bank, int64_t Cout, int64_t OW, bool has_bias);
bool emit_quarter_fold(Plan &plan, const std::string &name, const PlanOp &base, const DftBank &bank, const std::vector<int> &cls, int64_t Cout, int64_t OW,
                       bool has_bias);

#pragma GCC visibility pop
}  // namespace bn
