/*
 * ce_tp.h -- EXTENSION of libce_hip.so with NO counterpart in the reference: transform de-precoding (DFT-s-OFDM, the
 * inverse of TS 38.211 6.3.1.4) between ce_eq_equalize and ce_demod_demap, with the per-RE noise variances combined
 * into the per-symbol one the demapper needs.  Behind it, further down: transform precoding, the forward direction
 * (ce_tp_precode), OFDM demodulation, samples to the resource grid (ce_ofdm_*), which runs the same passes over the
 * same host view at the lengths 128 .. 4096, and OFDM modulation, the grid to samples, on the demodulator's plan
 * (ce_ofdmtx_modulate), between those two the time-domain channel emulator (ce_chan_apply), and the other front door, fronthaul
 * I/Q (de)compression between the wire format of an O-RAN 7.2x radio unit and the grid's rows (ce_fh_*), and behind that door
 * PRACH preamble detection over such rows (ce_prach_*) and SRS channel estimation over the grid's own rows (ce_srs_*), on the
 * same passes.
 *
 * The reference (pjookim/srsran-ce-pytorch) stops at the channel estimate.  The operator is pinned by the float64
 * restatement in tests/tp_oracle.py (`deprecode_ref`, against a literal M x M matrix form of 6.3.1.4) and the two
 * tolerance rules stated there.
 *
 * Transform precoding is single-layer and is used with DM-RS symbols that carry no data, so the equalizer's output
 * of such a slot is S = n_symbols rows of exactly M = 12 n_prbs entries: x_hat[slot][S M] complex64 and nvar[slot][S M]
 * float32, symbol ascending, subcarrier ascending (with intra-slot hopping both hops have the same n_prbs).  For one
 * layer the equalizer's x_hat_k = z / g is a per-RE zero-forcing estimate with nvar_k = 1 / g; a plain IDFT of it would
 * let one faded RE's noise flood the symbol and a single nvar_k = +inf erase it.  The operator is the MMSE
 * frequency-domain equalizer's combination, recovered from (x_hat, nvar) alone.  Per row (slot b, data symbol s),
 * k, i = 0 .. M - 1:
 *     usable_k = nvar_k finite and > 0, and both parts of x_hat_k finite
 *     beta_k   = 1 / (1 + nvar_k)        if usable_k, else 0     (the LMMSE weight g / (1 + g))
 *     gamma_k  = nvar_k / (1 + nvar_k)   if usable_k, else 1     (= 1 - beta_k, without the cancellation)
 *     u_k      = beta_k x_hat_k          if usable_k, else 0     (selected, never multiplied: no 0 * inf)
 *     mu       = (1 / M) sum_k beta_k
 *     t_i      = (1 / sqrt(M)) sum_k u_k exp(+j 2 pi i k / M)
 *     x_out_i    = t_i / mu
 *     nvar_out_i = (sum_k gamma_k) / (sum_k beta_k), the same value for every i of the row
 *     where sum_k beta_k = 0 (no usable RE):  x_out_i = 0, nvar_out_i = +inf   (the demapper's erasure convention)
 * x_out is unbiased (the coefficient of the transmitted x_i in t_i is mu); the residual inter-symbol interference plus
 * noise has variance mu (1 - mu) for unit-power symbols, hence nvar_out = (1 - mu) / mu.
 *
 * nvar_out is written broadcast over the row ([slot][S M] float32, the shape of x_out), so that ce_demod_demap consumes
 * both outputs unchanged: 4 M bytes written per row where 4 would do, a sixth of the pass's 24 M bytes per row.
 *
 * float32 arithmetic of the kernel (restated in tests/tp_oracle.py `deprecode_f32`): the two sums are taken in a fixed
 * order (threads_per_row partial sums, thread t over the REs 4 g .. 4 g + 3 of the groups g = t, t + threads_per_row,
 * .. in ascending order, then a balanced tree), so a row's result does not depend on the batch or on the row's place
 * in it; the transform is a Stockham mixed-radix FFT over the radix sequence of the host view with the twiddles
 * W[n] = exp(+j 2 pi n / M) computed on the host in float64 and rounded once; the output scale is sqrt(M) / sum_k beta_k.
 */
#ifndef CE_TP_H
#define CE_TP_H

#include "ce_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CE_TP_MAX_PRBS 275
#define CE_TP_MAX_PASSES 8 /* the longest radix sequence has 7 entries (e.g. M = 3240: 4 2 3 3 3 3 5) */

typedef struct ce_tp_desc {
  int32_t abi_version; /* = CE_ABI_VERSION */
  int32_t device;      /* HIP device ordinal the plan lives on */
  int32_t n_prbs;      /* 1 .. 275 of the form 2^a 3^b 5^c (38.211 6.3.1.4): M = 12 n_prbs */
  int32_t n_symbols;   /* S: data symbols per slot, 1 .. 14 */
} ce_tp_desc;

typedef struct ce_tp_plan ce_tp_plan; /* opaque */

typedef struct ce_tp_info {
  int32_t m_sc;           /* M */
  int32_t n_symbols;      /* S */
  int64_t bytes_per_slot; /* S M 24: x_hat and nvar in, x_out and nvar_out out */
} ce_tp_info;

/* What ce_tp_plan_create derives on the host. */
typedef struct ce_tp_host_view {
  int32_t m_sc;                         /* M */
  int32_t n_passes;                     /* entries of `radix` */
  int32_t radix[CE_TP_MAX_PASSES];      /* from {4, 2, 3, 5}, in pass order; their product is M */
  uint32_t stride_magic[CE_TP_MAX_PASSES]; /* pass p works at stride s_p = radix[0] .. radix[p-1]: floor(2^32 / s_p) + 1,
                                           so that floor(i / s_p) = (i * magic) >> 32 for i < M; 0 where s_p = 1 */
  int32_t threads_per_row;              /* 64, 128 or 256 */
  int32_t rows_per_workgroup;           /* 4, 2 or 1: threads_per_row * rows_per_workgroup = threads */
  int32_t threads;                      /* 256 */
  int32_t lds_bytes;                    /* rows_per_workgroup * 2 * 8 M: ping-pong buffers */
  int32_t twiddle_bytes;                /* 8 M */
  int32_t n_workgroups_per_slot;        /* ceil(S / rows_per_workgroup): a workgroup never spans two slots */
} ce_tp_host_view;

/* Validation and derivation of ce_tp_plan_create without touching a GPU: usable on a CPU-only host.
 * CE_ERR_INVALID: n_prbs outside 1..275 or with a prime factor above 5; n_symbols outside 1..14. */
int ce_tp_derive_host(const ce_tp_desc* desc, ce_tp_host_view* view);

/* Host only: the plan's twiddle table W[n] = exp(+j 2 pi n / M), n < M, as M (re, im) float32 pairs into `twiddles`
 * (twiddle_bytes of the host view). */
int ce_tp_copy_twiddles(const ce_tp_desc* desc, float* twiddles);

/* Validates the descriptor and uploads the twiddle table. */
int ce_tp_plan_create(const ce_tp_desc* desc, ce_tp_plan** out);
void ce_tp_plan_destroy(ce_tp_plan* plan);
int ce_tp_plan_get_info(const ce_tp_plan* plan, ce_tp_info* info);

/*
 * De-precoding of n_slots slots in ONE launch on `stream` (a hipStream_t; NULL = the default stream).  Asynchronous;
 * n_slots == 0 launches nothing.
 *  x_hat     [slot][S M] complex64, dense (ce_eq_equalize's x_hat of a one-layer slot)
 *  nvar      [slot][S M] float32, dense
 *  x_out     [slot][S M] complex64, dense; may be x_hat itself
 *  nvar_out  [slot][S M] float32, dense; may be nvar itself
 * In place is safe because a workgroup reads all of its rows before it writes any of them and no other workgroup
 * touches them; any other overlap between inputs and outputs is undefined.  All four pointers must be 16-byte aligned
 * (CE_ERR_INVALID otherwise); every row then is too, since 8 M and 4 M are multiples of 16, and every access to
 * the four tensors is 16 bytes wide.  No atomics, no scratch; every address comes from the block index, the thread index and
 * host-derived plan values, tensor values enter arithmetic only.
 */
int ce_tp_deprecode(const ce_tp_plan* plan, const void* x_hat, const float* nvar, int64_t n_slots, void* x_out, float* nvar_out,
                    void* stream);

/*
 * Transform PRECODING, TS 38.211 6.3.1.4 itself (the transmit side: behind ce_mod_modulate), of n_slots slots in ONE
 * launch on `stream`, with the plan of the same n_prbs and n_symbols: radix sequence, stride constants, twiddle table
 * and launch geometry are the de-precoder's.  Asynchronous; n_slots == 0 launches nothing.  For slot b < n_slots,
 * row r < S and k, i < M, complex64, strides and offsets in complex elements:
 *     y[b y_slot_stride + y_row_offset[r] + k] = (1 / sqrt(M)) sum_i x[b x_slot_stride + x_row_offset[r] + i] exp(-j 2 pi i k / M)
 * the sign and the scale of tests/tp_oracle.py `precode`.
 *  x_row_offset, y_row_offset   host memory, S int32 each, read during the call (they travel in the kernel arguments);
 *                               NULL = dense rows, r M.  With the rows of a resource grid [slot][n_sym][n_sc] (what
 *                               ce_mod_modulate writes for one layer) the offset of the data symbol s is
 *                               s n_sc + 12 prb_start and the slot stride n_sym n_sc.
 * CE_ERR_INVALID unless: x and y are 16-byte aligned; both strides and every offset are even and >= 0 (every row then
 * is 16-byte aligned, and every access to x and y is 16 bytes wide); offset + M <= slot stride for every row; the
 * rows of one slot are pairwise disjoint, in x and in y; and x and y do not overlap -- except that y may be x itself
 * with the identical stride and offsets, the in-place form (a grid is transformed where it lies).  The extent of a
 * tensor is (n_slots - 1) stride + max offset + M elements.  In place is safe for the de-precoder's reason: a workgroup
 * loads all of its rows before its first barrier, stores them after its last, and no other workgroup touches them.
 * CE_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups in one launch.
 *
 * float32 arithmetic (restated in tests/tpre_oracle.py `precode_f32`): the forward transform is the plan's inverse
 * transform between two conjugations, DFT(x) = conj(IDFT(conj(x))).  The conjugation on load and the one on store flip
 * a sign bit and are exact; between them run the de-precoder's Stockham passes over the same radix sequence with the same
 * twiddles W[n] = exp(+j 2 pi n / M); the last pass scales by float32(1 / sqrt(M)), computed on the host in double and
 * rounded once.  No reduction and no special-value handling: a NaN or an infinity in a row stays in that row and
 * reaches no other.  No atomics, no scratch; every address comes from the block index, the thread index and host-derived
 * values.  The pass moves 16 S M bytes per slot (x in, y out); ce_tp_info.bytes_per_slot keeps the de-precoder's 24 S M.
 */
int ce_tp_precode(const ce_tp_plan* plan, const void* x, int64_t x_slot_stride, const int32_t* x_row_offset, void* y,
                  int64_t y_slot_stride, const int32_t* y_row_offset, int64_t n_slots, void* stream);

/*
 * OFDM DEMODULATION, the receive side in front of the estimator: time-domain I/Q samples of a slot to the resource grid
 * received_rg -- cyclic-prefix removal, a DFT of length N = 2^n per symbol with the transforms' Stockham passes, the
 * mapping of the bins onto the grid's subcarriers, compensation of the window advance and the per-symbol phase of
 * TS 38.211 5.4.  The entry points take scalars and pointers only; the one structure is ce_tp_host_view, which describes
 * an N-point transform as it stands: m_sc holds N, radix / stride_magic / threads_per_row / rows_per_workgroup / threads /
 * lds_bytes / twiddle_bytes keep their meaning, and n_workgroups_per_slot counts the workgroups of one (slot, port).
 *
 * Plan values:
 *     n_fft = N            128, 256, 512, 1024, 2048 or 4096
 *     n_prb_grid           n_sc = 12 n_prb_grid <= N
 *     n_sym                1 .. 14
 *     cp_len[n_sym]        int32, samples, >= 0 (host memory, read during the call)
 *     window_advance = a   0 <= a <= min cp_len: the DFT window starts a samples inside the cyclic prefix
 *     sym_phasor           n_sym (re, im) float32 pairs phi_l, all finite (host memory), or NULL for none
 * Derived: the slot length T = sum_l (cp_len[l] + N); the symbol start t_l = sum_{i<l} (cp_len[i] + N); the window start
 * w_l = t_l + cp_len[l] - a; the signed bin of the grid subcarrier k < n_sc, q_k = k - n_sc / 2 (no k0 offset), at the
 * transform's bin q_k mod N.  For slot b, port r, symbol l, with s = samples + b slot_stride + r port_stride:
 *     Y[b][r][l][k] = phi_l exp(+j 2 pi q_k a / N) N^(-1/2) sum_{n<N} s[w_l + n] exp(-j 2 pi q_k n / N)
 * The scale is unitary.  With a transmitter that puts X_k on bin q_k with the same scale and a channel shorter than
 * min cp_len - a samples, Y = H_k X_k.
 *
 * float32 arithmetic (restated in tests/ofdm_oracle.py `demodulate_f32`): the forward transform is the inverse one between
 * two conjugations, as in ce_tp_precode -- conjugate on load (exact), the Stockham passes over the radix sequence of the
 * host view with the twiddles W[n] = exp(+j 2 pi n / N) computed in double and rounded once, the last pass scaling by
 * float32(1 / sqrt(N)), conjugate on store (exact).  At the store the value v of bin q_k mod N is multiplied, in this
 * order and each only where it applies, by
 *     1. W[(q_k a) mod N]     where a != 0: a lookup in the plan's own twiddle table, the index in integer arithmetic
 *     2. phi_l                where sym_phasor was given
 * each a complex product (v.re w.re - v.im w.im, v.re w.im + v.im w.re).  With a = 0 and no phasors the result is the bare
 * scaled DFT.  No reduction and no special-value handling: a NaN or an infinity in a window stays in that window's row.
 *
 *  samples   complex64 [slot][port][>= T], the last dimension contiguous; slot_stride and port_stride in complex
 *            elements, any values >= 0 (a view into a longer capture; 0 repeats a row).  8-byte aligned, read with 8-byte
 *            loads: cyclic prefixes such as 9 or 10 samples put windows at odd offsets.  Only the N samples of each of the
 *            n_sym windows are read.
 *  out       complex64 [slot][port][n_sym][n_sc], dense, 16-byte aligned, written with 16-byte stores, every element
 *            exactly once: the estimator's fast layout, of which received_rg[B, R, n_sc, n_sym] is the permuted view.
 * One launch on `stream`, asynchronous; n_slots == 0 or n_ports == 0 launches nothing.  One 256-thread workgroup handles
 * rows_per_workgroup windows of one (slot, port); two LDS buffers of N complex64 per window.  No atomics, no scratch;
 * every address comes from the block index, the thread index and host-derived values.
 * CE_ERR_INVALID: n_fft not one of the six sizes; n_sc > N; n_sym outside 1..14; a negative cp_len; a outside
 * 0 .. min cp_len; a non-finite phasor; a negative stride or count; strides whose extent exceeds the address space;
 * samples not 8-byte or out not 16-byte aligned; out overlapping the extent
 * (n_slots - 1) slot_stride + (n_ports - 1) port_stride + T of samples.
 * CE_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups in one launch.
 */
typedef struct ce_ofdm_plan ce_ofdm_plan; /* opaque */

/* Host only: validation and derivation of ce_ofdm_plan_create without touching a GPU. */
int ce_ofdm_derive_host(int32_t n_fft, int32_t n_prb_grid, int32_t n_sym, const int32_t* cp_len, int32_t window_advance,
                        ce_tp_host_view* view);

/* Host only: the plan's twiddle table W[n] = exp(+j 2 pi n / N), n < N, as N (re, im) float32 pairs into `twiddles`. */
int ce_ofdm_copy_twiddles(int32_t n_fft, float* twiddles);

/* Validates the values and uploads the twiddle table to `device`; abi_version = CE_ABI_VERSION. */
int ce_ofdm_plan_create(int32_t abi_version, int32_t device, int32_t n_fft, int32_t n_prb_grid, int32_t n_sym, const int32_t* cp_len,
                        int32_t window_advance, const float* sym_phasor, ce_ofdm_plan** out);
void ce_ofdm_plan_destroy(ce_ofdm_plan* plan);

int ce_ofdm_demodulate(const ce_ofdm_plan* plan, const void* samples, int64_t slot_stride, int64_t port_stride, int64_t n_slots,
                       int64_t n_ports, void* out, void* stream);

/*
 * OFDM MODULATION, the transmit side behind ce_mod_modulate (and ce_tp_precode): the resource grid to the time-domain
 * samples of a slot, on a ce_ofdm_plan -- the mapping of the grid's subcarriers onto the bins around DC, a transform of
 * length N per symbol with the same Stockham passes, radix sequence, twiddle table and launch geometry as the
 * demodulator, and the cyclic prefix in front of every symbol.  The plan's window_advance is a receiver value and is
 * ignored.  For slot b, port r, symbol l and n = -cp_len[l] .. N - 1, with s = samples + b slot_stride + r port_stride:
 *     s[t_l + cp_len[l] + n] = N^(-1/2) sum_{k<n_sc} conj(phi_l) X[b][r][l][k] exp(+j 2 pi q_k n / N)
 * the operator of tests/ofdm_oracle.py `modulate`.  The scale is unitary; phi_l is the plan's sym_phasor, the
 * DEMODULATOR's value, of which the modulator applies the conjugate, and only where phasors were given.  So
 * ce_ofdm_demodulate with the same plan values returns X through an ideal channel, for any advance a <= min cp_len.
 * One grid row per port: there is no layer-to-port precoding matrix, no windowing or overlap-add between symbols.
 *
 * float32 arithmetic (restated in tests/ofdm_tx_oracle.py `modulate_f32`): where phasors were given, X is multiplied by
 * (phi_l.re, -phi_l.im) -- the sign flip is exact -- as the complex product (x.re w.re - x.im w.im, x.re w.im + x.im w.re);
 * the value goes to bin q_k mod N and the other N - n_sc bins are zero; the passes are the inverse transform natively, so
 * there is no conjugation; the last pass scales by float32(1 / sqrt(N)); the cyclic prefix is the symbol's last
 * cp_len[l] values stored a second time, bit for bit.  No reduction and no special-value handling: a NaN or an infinity
 * in a symbol of the grid stays in the cp_len[l] + N samples of that symbol.
 *
 *  grid      complex64 [slot][port][n_sym][n_sc], dense, 16-byte aligned, read with 16-byte loads (what ce_mod_modulate
 *            writes and ce_ofdm_demodulate returns).
 *  samples   complex64, row (b, r) at b slot_stride + r port_stride, strides in complex elements (a view into a longer
 *            stream); 8-byte aligned, written with 8-byte stores: cyclic prefixes such as 9 or 10 samples put symbols at
 *            odd offsets.  Every sample of [0, T) of every row is written exactly once, nothing else.
 * One launch on `stream`, asynchronous; n_slots == 0 or n_ports == 0 launches nothing, whatever the pointers.  One
 * 256-thread workgroup handles rows_per_workgroup symbols of one (slot, port).  No atomics, no scratch; every address
 * comes from the block index, the thread index and host-derived values.
 * CE_ERR_INVALID: a null plan (refused first) or pointer; a negative count or stride; grid not 16-byte or samples not
 * 8-byte aligned; strides whose extent exceeds the address space; rows of samples that are not pairwise disjoint --
 * accepted are the ports inside a slot (port_stride >= T where n_ports > 1, slot_stride >= (n_ports - 1) port_stride + T
 * where n_slots > 1) and the slots inside a port, one continuous stream per port (slot_stride >= T where n_slots > 1,
 * port_stride >= (n_slots - 1) slot_stride + T where n_ports > 1); the extent
 * (n_slots - 1) slot_stride + (n_ports - 1) port_stride + T of samples overlapping grid.
 * CE_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups in one launch.
 */
int ce_ofdmtx_modulate(const ce_ofdm_plan* plan, const void* grid, int64_t n_slots, int64_t n_ports, void* samples,
                       int64_t slot_stride, int64_t port_stride, void* stream);

/*
 * TIME-DOMAIN CHANNEL EMULATOR between ce_ofdmtx_modulate and ce_ofdm_demodulate: a FIR channel from n_tx transmit to n_rx
 * receive ports, a carrier frequency offset from a numerically controlled oscillator, and seeded white Gaussian noise, in
 * ONE launch on `stream` of the CURRENT device, without a plan.  Scalars and pointers only.  For slot b < n_slots = B, receive
 * port r < n_rx = R, sample t < n_samples = T, with P = n_tx, K = n_taps (the float64 operator of tests/chan_oracle.py
 * `apply_ref`):
 *     y[b][r][t] = exp(j 2 pi w_b(t) / 2^32) sum_{p<P} sum_{k<K} h[b][r][p][k] x[b][p][t - k]  +  sigma_b n[b][r][t]
 * with x[b][p][t - k] = 0 for t - k < 0: every slot row is convolved on its own (np.convolve(..)[:T]), the tail of slot b does
 * not run into slot b + 1.
 *   CFO    w_b(t) = (phase0_b + fcw_b t) mod 2^32 in uint32 arithmetic, t counted from the row's start: fcw is an int32
 *          frequency in units of 2^-32 cycles per sample (+-half the sample rate), phase0 a uint32.  The phase word is exact;
 *          the kernel turns it into a phasor as sincospi(float32(int32(w)) 2^-31).  fcw == NULL: no rotation at all.
 *   noise  n has unit power E|n|^2 = 1 and comes from Philox4x32-10 (multipliers D2511F53, CD9E8D57, Weyl constants
 *          9E3779B9, BB67AE85) with the key (seed & 0xffffffff, seed >> 32) and the counter
 *          (t >> 1, r, s & 0xffffffff, s >> 32), s = first_slot + b: one call gives the four words of the samples 2 i and
 *          2 i + 1, (w0, w1) for 2 i and (w2, w3) for 2 i + 1.  Of a word pair (a, c): u1 = ((a >> 8) + 1) 2^-24 in (0, 1],
 *          u2 = (c >> 8) 2^-24, n = sqrt(-ln u1) exp(j 2 pi u2).  So the noise of a sample depends on (seed, first_slot + b,
 *          r, t) alone: not on the batch, the launch geometry, x or h.  sigma == NULL: no noise and no Philox call.
 *
 *  x        complex64 [slot][tx port][>= T], the last dimension contiguous, x_slot_stride and x_port_stride in complex
 *           elements, any values >= 0 (a view into a longer stream, what ce_ofdmtx_modulate writes); 8-byte aligned, read with
 *           8-byte loads.  Only [0, T) of each row is read.
 *  taps     complex64 [slot][R][P][K], dense behind taps_slot_stride (complex elements): >= R P K, or 0 for one channel for
 *           the whole batch.  8-byte aligned.
 *  fcw, phase0, sigma   DEVICE memory, one int32 / uint32 / float32 per slot at b stride; stride 0: one value for the batch.
 *           phase0 is read only where fcw is given.  sigma >= 0.
 *  y        complex64, row (b, r) at b y_slot_stride + r y_port_stride; 8-byte aligned, written with 8-byte stores.  Every
 *           sample of [0, T) of every row is written exactly once, nothing else.
 * Asynchronous; n_slots == 0 launches nothing.  One 256-thread workgroup per (slot, rx port, tile of 1024 samples) stages
 * the tile and its n_taps - 1 predecessors of every tx port in LDS (at most 40 KiB).  float32 arithmetic (restated in
 * tests/chan_oracle.py `apply_f32`): FMAs in the fixed order p outer, k inner, per product re += h.re x.re,
 * re -= h.im x.im, im += h.re x.im, im += h.im x.re; then the phasor (c, s): (fma(re, c, -(im s)), fma(re, s, im c)); then
 * fma(sigma, n.re, .) and fma(sigma, n.im, .) with n = (rad cos, rad sin), rad = sqrtf(-logf(u1)), sincospi(2 u2).  No
 * atomics, no scratch; every address and bound comes from the block index, the thread index and the scalars of the call.
 * A NaN in x[b][p][t] reaches y[b][:][t .. t + K - 1] and nothing else.
 * CE_ERR_INVALID: abi_version != CE_ABI_VERSION; n_tx outside 1..4, n_taps outside 1..128, n_rx < 1, n_samples < 1; a
 * negative count or stride; a null x, y or taps (or fcw without phase0) in a non-empty batch; x, y or taps not 8-byte
 * aligned; strides whose extent exceeds the address space; a taps_slot_stride between 1 and R P K - 1; rows of y that are
 * not pairwise disjoint (ce_ofdmtx_modulate's conditions on its samples); the extent of y overlapping that of x or of taps.
 * CE_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups in one launch.
 */
int ce_chan_apply(int32_t abi_version, const void* x, int64_t x_slot_stride, int64_t x_port_stride, int64_t n_slots, int32_t n_tx,
                  int64_t n_rx, int64_t n_samples, const void* taps, int64_t taps_slot_stride, int32_t n_taps, const int32_t* fcw,
                  int64_t fcw_stride, const uint32_t* phase0, int64_t phase0_stride, const float* sigma, int64_t sigma_stride,
                  uint64_t seed, int64_t first_slot, void* y, int64_t y_slot_stride, int64_t y_port_stride, void* stream);

/* Host only: the four Philox words of the sample pair t_pair = t >> 1 of (slot = first_slot + b, rx port), as the kernel
 * draws them: counter (t_pair, port, slot low, slot high), each truncated to 32 bits, key (seed low, seed high). */
int ce_chan_noise_words(uint64_t seed, int64_t slot, int32_t port, int64_t t_pair, uint32_t out[4]);

/*
 * FRONTHAUL I/Q (DE)COMPRESSION, the front door behind an O-RAN 7.2x radio unit, which does the FFT itself: the
 * frequency-domain I/Q of one (port, symbol) as it travels (O-RAN.WG4.CUS Annex A.1 and the udCompParam byte) to and from
 * rows of the resource grid, each direction in ONE launch on `stream` of the CURRENT device, without a plan.  Scalars and
 * pointers only.  Every output is defined to the bit (restated bit-serially in tests/fh_oracle.py).
 *
 * A row carries n_prb PRBs one after the other without padding, row_bytes = n_prb prb_bytes in all (ce_fh_row_bytes).
 *   CE_FH_BFP, mantissa width W = iq_width in 1..16: prb_bytes = 1 + 3 W.  Byte 0 is the compression parameter: its low 4
 *       bits the exponent e in 0..15, its high 4 bits reserved (ignored by the decompressor, 0 from the compressor).  Then
 *       the 24 mantissas I0, Q0, I1, Q1, .., I11, Q11, each W bits of two's complement, packed MSB first without gaps: bit 7
 *       of byte 1 is the top bit of I0.
 *   CE_FH_NONE: prb_bytes = 48, the 24 values as big-endian int16 in the same order and no parameter byte -- CE_FH_BFP with
 *       W = 16, e = 0 and no byte 0.  iq_width must still lie in 1..16 and is otherwise ignored.
 * Decompression: v = sign_extend(mantissa) << e as int32 (|v| <= 2^30 with at most 16 significant bits, so float(v) is
 * exact); the component is float(v) * scale, one float32 multiply.
 * Compression of a float32 component x: q = x * inv_scale (one float32 multiply; the caller passes
 * inv_scale = float32(1 / double(scale))), v = rintf(q) to the nearest even, NaN -> 0, saturated to -32768 .. 32767 (the
 * infinities saturate).  Per PRB, over its 24 values: mag = v >= 0 ? v : ~v, L = bit_length(max mag) (0 for 0),
 * e = max(L + 1 - W, 0), mantissa = v >> e, an arithmetic shift (a floor); CE_FH_NONE stores v.  Hence e <= 15, every
 * mantissa fits W bits, 0 <= v - (mantissa << e) < 2^e, and compressing mantissa << e gives (e, mantissa) again.
 * scale and inv_scale: float32 in 2^-96 .. 2^96 (no product is denormal or overflows).
 *
 *  payload  uint8, row (b, r, y) at b slot + r port + y symbol stride, strides in BYTES; the base and the three strides
 *           multiples of 4.  Read (ce_fh_decompress) with dword loads except a row's last row_bytes mod 4 bytes, which are
 *           read one by one: no byte behind row_bytes is touched.  Written (ce_fh_compress) with dword stores and byte
 *           stores for that tail: bytes between row_bytes and the next row are NOT written.
 *  grid     complex64, 8-byte aligned: the first RE of the first PRB of row (0, 0, 0); row (b, r, y) at b slot + r port +
 *           y symbol stride, strides in complex64 elements (any parity), subcarriers contiguous -- the estimator's fast
 *           layout [slot][port][symbol][subcarrier], of which a PRB range is a section.  The 12 n_prb REs of every row are
 *           written (read) exactly once, nothing else; 16-byte accesses where the base and the strides keep every row on
 *           16 bytes, 8-byte accesses otherwise.
 * One 256-thread workgroup per (slot, port, symbol, tile of 64 PRBs); at most 3.3 KiB of LDS.  No atomics, no scratch;
 * payload and grid values enter arithmetic only: every address and bound comes from the block index, the thread index
 * and the scalars of the call.  Asynchronous; n_slots == 0 launches nothing, whatever the pointers.
 * CE_ERR_INVALID: abi_version != CE_ABI_VERSION; iq_width outside 1..16; n_prb outside 1..341; n_sym < 1; n_ports < 1;
 * n_slots < 0; a scale outside 2^-96 .. 2^96 or not finite; a null pointer in a non-empty batch; a negative stride; a
 * payload base or stride that is no multiple of 4; a grid that is not 8-byte aligned; strides whose extent exceeds the
 * address space; rows of the WRITTEN side that are not pairwise disjoint (accepted: by ascending stride, each stride of a
 * dimension with more than one entry at least the extent of everything inside it -- any nesting of slot, port and symbol;
 * the strides of the side that is read are free, 0 repeats a row); the extents of payload and grid overlapping.
 * CE_ERR_UNSUPPORTED: an unknown method; more than 2^31 - 1 workgroups in one launch.
 */
#define CE_FH_NONE 0
#define CE_FH_BFP 1
#define CE_FH_MAX_PRBS 341

/* Host only: the bytes of a row of n_prb PRBs, n_prb (1 + 3 iq_width) or 48 n_prb, into *bytes. */
int ce_fh_row_bytes(int32_t method, int32_t iq_width, int32_t n_prb, int64_t* bytes);

int ce_fh_decompress(int32_t abi_version, const void* payload, int64_t payload_slot_stride, int64_t payload_port_stride,
                     int64_t payload_symbol_stride, void* grid, int64_t grid_slot_stride, int64_t grid_port_stride,
                     int64_t grid_symbol_stride, int64_t n_slots, int64_t n_ports, int32_t n_sym, int32_t n_prb, int32_t method,
                     int32_t iq_width, float scale, void* stream);

int ce_fh_compress(int32_t abi_version, void* payload, int64_t payload_slot_stride, int64_t payload_port_stride,
                   int64_t payload_symbol_stride, const void* grid, int64_t grid_slot_stride, int64_t grid_port_stride,
                   int64_t grid_symbol_stride, int64_t n_slots, int64_t n_ports, int32_t n_sym, int32_t n_prb, int32_t method,
                   int32_t iq_width, float inv_scale, void* stream);

/*
 * PRACH PREAMBLE DETECTION over frequency-domain rows, the other kind of uplink I/Q an O-RAN 7.2x radio unit sends (section
 * type 3): per PRACH occasion and Zadoff-Chu root the correlation with the root in the frequency domain, an inverse transform
 * of length N with the transforms' Stockham passes, the power delay profile summed over ports and repetitions, and per
 * cyclic-shift window its maximum and where it lies.  Short formats (L_RA = 139, also 571 and 1151) and long formats
 * (L_RA = 839) alike; the 1.25 kHz time-domain front end (decimation, long FFT) stays with the radio unit.  The entry points
 * take scalars and pointers only; the one structure is ce_tp_host_view, which describes the N-point transform as it stands
 * (m_sc holds N, n_workgroups_per_slot is 1: one workgroup per (occasion, root)).
 *
 * Plan values:
 *     l_ra = L             139, 571, 839 or 1151 (odd primes)
 *     n_fft = N            256, 512, 1024, 2048 or 4096, N > L
 *     n_roots, roots[]     1 .. 64 distinct PHYSICAL root indices u_i in 1 .. L - 1 (host int32, read during the call).  The
 *                          logical-to-physical table of TS 38.211 Tables 6.3.3.1-3/-4 is the caller's data.
 *     n_cs                 0 .. L - 1, the cyclic-shift step N_CS (unrestricted set)
 *     n_shifts             1 .. 64 windows per root, n_shifts n_cs <= L; n_cs = 0 requires n_shifts = 1
 *     combine              0: repetitions are combined non-coherently, 1: coherently
 * Derived on the host, in integers: the guard g = ceil(N / L); the shift C_v = v n_cs, v < n_shifts; for n_cs > 0
 *     win_start[v] = (floor(((L - C_v) mod L) N / L) - g) mod N        win_len = floor(n_cs N / L)
 * and for n_cs = 0 win_start[0] = 0, win_len = N.  The windows are pairwise disjoint (floor(x) - floor(x - y) >= floor(y));
 * window 0 always wraps round N.  A preamble of shift C_v that arrives without delay peaks at the fractional index
 * ((L - C_v) mod L) N / L; the guard keeps the main lobe of such a preamble out of the tail of the neighbouring window.
 *
 * Root table, TS 38.211 6.3.3.1: x_u(n) = exp(-j 2 pi ((u n (n + 1) / 2) mod L) / L), the index reduced in integers;
 * X_u[k] = sum_{n<L} x_u(n) exp(-j 2 pi n k / L); T_i[k] = conj(X_{u_i}[k]) / |X_{u_i}[k]|, k < L, in double on the host and
 * rounded once to float32.  (For odd prime L, X_u[k] = X_u[0] conj(x_u(u^-1 k mod L)): the host takes the sum once per root.)
 *
 * Per occasion b and root i a TERM is (port r, repetition s) with Z[k] = Y[b][r][s][k] T_i[k] when combine = 0, and a port r
 * with Z[k] = (sum_s Y[b][r][s][k]) T_i[k], summed over s ascending, when combine = 1.  Then, for n < N:
 *     z[n]           = (1 / L) sum_{k<L} Z[k] exp(+j 2 pi k n / N)         (bin k -> k, the other N - L bins zero)
 *     P[b][i][n]     = sum over the terms of |z[n]|^2
 *     mean[b][i]     = (1 / N) sum_n P[b][i][n]
 *     peak[b][i][v]  = max_{d < win_len} P[b][i][(win_start[v] + d) mod N]
 *     delay[b][i][v] = the smallest d that attains it
 * A noiseless preamble of amplitude a on one port, aligned to the N grid, gives peak = a^2.  Detection is
 * peak / mean > threshold and belongs to the caller.  Preamble (i, v) arrived
 * (win_start[v] + delay - ((L - C_v) mod L) N / L) / (N delta_f_RA) seconds late: the fractional window start is put back on
 * the host.
 *
 * float32 arithmetic (restated in tests/prach_oracle.py `detect_f32`): the coherent sum over s in ascending order starting
 * from Y[..][0]; the product (y.re t.re - y.im t.im, y.re t.im + y.im t.re); the passes of the transforms (the inverse
 * transform natively: no conjugation) over the radix sequence of the host view with the twiddles W[n] = exp(+j 2 pi n / N),
 * the last pass scaling by float32(1 / L), computed in double and rounded once; re re + im im per term.  Row q of the
 * workgroup's rows_per_workgroup rows sums its terms q, q + rows_per_workgroup, .. in ascending order, starting from 0; the rows
 * are then added in ascending row order.  The sum for mean: thread t < 256 adds P[t], P[t + 256], .. in ascending order, a
 * butterfly of lane exchanges (distances 32, 16, .., 1) per wave, the four waves as (w0 + w1) + (w2 + w3), times 1 / N
 * (exact).  An occasion's outputs do not depend on the batch it is in, a root's not on the other roots of the plan.  A NaN or
 * an infinity in an occasion stays in that occasion; a window that holds no ordered value reports peak NaN and delay 0.
 *
 *  y        complex64, row (b, r, s) at b occasion_stride + r port_stride + s rep_stride, strides in complex elements, any
 *           values >= 0 (a view of the decompressor's grid [slot][port][symbol][subcarrier]; 0 repeats a row); 8-byte
 *           aligned, read with 8-byte loads.  Only the L elements of each row are read.
 *  peak     float32 [B][n_roots][n_shifts], delay int32 of the same shape, mean float32 [B][n_roots], and the optional
 *           profile float32 [B][n_roots][N] (NULL: not written): dense, 4-byte aligned, every element written exactly once.
 * One launch on `stream`, asynchronous; n_occasions == 0 launches nothing, whatever the pointers.  One 256-thread workgroup
 * per (occasion, root) loops over the item's terms, rows_per_workgroup at a time; two LDS buffers of N complex64 per row.  No
 * atomics, no scratch; every address comes from the block index, the thread index and host-derived values.
 * CE_ERR_INVALID: abi_version != CE_ABI_VERSION; l_ra or n_fft not in the lists, or n_fft <= l_ra; n_roots or n_shifts outside
 * 1..64; a root outside 1 .. L - 1 or listed twice; n_cs outside 0 .. L - 1; n_shifts n_cs > L; n_cs = 0 with n_shifts > 1;
 * combine not 0 or 1; a null argument; n_occasions < 0, n_ports outside 1..64, n_reps outside 1..12; a negative stride;
 * strides whose extent exceeds the address space; y not 8-byte or an output not 4-byte aligned; an output overlapping the
 * extent (B - 1) occasion_stride + (n_ports - 1) port_stride + (n_reps - 1) rep_stride + L of y.
 * CE_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups in one launch.
 */
typedef struct ce_prach_plan ce_prach_plan; /* opaque */

/* Host only: validation and derivation of ce_prach_plan_create without touching a GPU: the view of the N-point transform,
 * the n_shifts window starts into `win_start` and the common window length into *win_len. */
int ce_prach_derive_host(int32_t l_ra, int32_t n_fft, int32_t n_roots, const int32_t* roots, int32_t n_cs, int32_t n_shifts,
                         int32_t combine, ce_tp_host_view* view, int32_t* win_start, int32_t* win_len);

/* Host only: the plan's tables as (re, im) float32 pairs: the N twiddles W[n] = exp(+j 2 pi n / N) into `twiddles` and the
 * n_roots x L root table T_i[k] into `table`; either may be NULL and is then left out. */
int ce_prach_copy_tables(int32_t l_ra, int32_t n_fft, int32_t n_roots, const int32_t* roots, float* twiddles, float* table);

/* Validates the values and uploads the twiddles and the root table to `device`; abi_version = CE_ABI_VERSION. */
int ce_prach_plan_create(int32_t abi_version, int32_t device, int32_t l_ra, int32_t n_fft, int32_t n_roots, const int32_t* roots,
                         int32_t n_cs, int32_t n_shifts, int32_t combine, ce_prach_plan** out);
void ce_prach_plan_destroy(ce_prach_plan* plan);

int ce_prach_detect(const ce_prach_plan* plan, const void* y, int64_t occasion_stride, int64_t port_stride, int64_t rep_stride,
                    int64_t n_occasions, int32_t n_ports, int32_t n_reps, float* peak, int32_t* delay, float* mean,
                    float* profile /* may be NULL */, void* stream);

/*
 * SRS CHANNEL ESTIMATION over the frequency-domain grid rows of the sounding reference signal (TS 38.211 6.4.1.4), the third
 * kind of uplink I/Q in a section-type-1 grid: per item and receive port the power delay profile of the sounding ports
 * (ce_srs_profile), and, with a delay taken out, the channel per sounding port and 4-PRB block, its wideband mean, the noise
 * and the received energy (ce_srs_estimate).  Two launches; the delay between them is the caller's (the wrapper's argmax, on
 * the device).  Scalars and pointers only; the one structure is ce_tp_host_view of the N-point transform (m_sc holds N,
 * n_workgroups_per_slot is 1: one workgroup per (item, receive port)).
 *
 * Plan values:
 *     k_tc                 2 or 4: the comb.  n_cs_max = 8 (comb 2) or 12 (comb 4)
 *     n_ap                 1, 2 or 4 sounding ports;  n_cs in 0 .. n_cs_max - 1;  k_bar in 0 .. k_tc - 1
 *     m_srs                PRBs per symbol, a multiple of 4 in 4 .. 272
 *     n_symb, l0           1, 2 or 4 consecutive symbols from l0 inside the grid's n_sym <= n_symb_slot (12 or 14) symbols
 *     start_prb[n_symb]    per symbol, start_prb[s] + m_srs <= n_prb_grid (<= 341).  Frequency hopping is the caller's: the
 *                          C_SRS / B_SRS table 6.4.1.4.3-1 is the caller's data (host int32, read during the call)
 *     hopping              CE_DMRS_LP_HOP_NEITHER / _GROUP / _SEQUENCE of ce_dmrs.h;  slots_per_frame 10, 20, 40, 80 or 160
 *     n_fft = N            128, 256, 512, 1024, 2048 or 4096, N > M
 *     win_len              1 .. N indices of the profile
 *     phi                  int8 [30][M] of -3, -1, 1, 3 where M is 12 or 24 (38.211 Tables 5.2.2.2-1/-2: caller data; NULL
 *                          is CE_ERR_UNSUPPORTED there), ignored otherwise
 * Derived on the host, in integers: M = 12 m_srs / k_tc sequence elements; a block is 4 PRB = Q = 48 / k_tc elements (a
 * multiple of n_cs_max: the ports of a comb are exactly orthogonal over a block); n_blocks = m_srs / 4; the guard
 * g = ceil(N / M); per port i < n_ap
 *     cs_i = (n_cs + n_cs_max i / n_ap) mod n_cs_max, comb_i = k_bar, except for n_ap = 4 with n_cs >= n_cs_max / 2:
 *     cs_i = (n_cs + n_cs_max floor(i / 2) / 2) mod n_cs_max, and ports 1 and 3 on comb (k_bar + k_tc / 2) mod k_tc;
 * the used combs (n_combs = 1 or 2) in the order of their first port.  The default window of the wrapper is
 * floor(N gap / n_cs_max) - g with gap = n_cs_max / (ports on the fullest comb).
 *
 * Sequence: rbar_{u,v}(n), n < M, is the low-PAPR base sequence of 5.2.2 exactly as ce_dmrs_lp_* derive it (ce_dmrs.h): for
 * M >= 36 W_{N_ZC}[(q[u][v] tri[n]) mod N_ZC] with N_ZC the largest prime below M, for M = 12, 24 exp(j phi_u(n) pi / 4);
 * M = 30 cannot occur.  Hopping per symbol p = n_symb_slot (slot mod slots_per_frame) + l0 + s: u = (f_gh + n_id) mod 30,
 * group hopping f_gh = (sum_{m<8} 2^m c(8 p + m)) mod 30, sequence hopping v = c(p) where M >= 72, with c_init = n_id IN
 * BOTH MODES (6.4.1.4.2; PUSCH's group hopping has floor(n_id / 30)).  Port i transmits rbar(n) rho_i[n],
 * rho_i[n] = exp(+j 2 pi cs_i n / n_cs_max) (a table of n_cs_max values per port, computed in double and rounded once), on
 * the subcarriers k(s, comb_i, n) = 12 start_prb[s] + comb_i + k_tc n of symbol l0 + s.
 *
 * ce_srs_profile, per item b and receive port r, the TERMS (s, i) in the order s outer, i inner:
 *     G_i[n]   = y[b][r][l0 + s][k(s, comb_i, n)] conj(rbar(n)) conj(rho_i[n])
 *     z[d]     = (1 / M) sum_{n<M} G_i[n] exp(+j 2 pi n d / N)
 *     profile[b][r][d'] = sum over the terms of |z[(d' - g) mod N]|^2,  d' < win_len
 * A flat unit channel with gains h and no delay puts sum |h|^2 at d' = g.  The delay of an item is
 * argmax_d' sum_r profile[b][r][d'] - g on the N grid, delay / (N k_tc scs) seconds: torch operations of the wrapper.
 *
 * ce_srs_estimate, with d = delay[b] mod N (NULL: 0; any int32, it cannot address memory), the compensation
 * w[n] = W_N[(n d) mod N] gathered from the plan's twiddles W_N[e] = exp(+j 2 pi e / N), and per used comb c
 *     g_c[n] = (y[b][r][l0 + s][k(s, c, n)] conj(rbar(n))) w[n]
 *     h_sb[b][r][i][s][j] = (1 / Q) sum_{n in block j, ascending} g_{comb_i}[n] conj(rho_i[n])
 *     h_wb[b][r][i]       = the mean of h_sb over (s, j), s outer
 *     e_c[n]              = g_c[n] - sum_{i: comb_i = c, ascending} h_sb[b][r][i][s][j(n)] rho_i[n]
 *     noise[b][r]         = sum_{s,c,n} |e_c[n]|^2 / (n_symb n_combs M - n_symb n_ap M / Q)
 *     epre[b][r]          = the mean of |y|^2 over the same resource elements
 * The noise comes from the residual itself, never from the difference of two energies.  h_sb is referred to each symbol's
 * first comb element: the constant phase exp(-j 2 pi (12 start_prb[s] + comb_i) delay / (N k_tc)) of a delayed channel stays
 * in it (the wrapper's srs_band_response puts it back).
 *
 * float32 arithmetic (restated in tests/srs_oracle.py): a conj(b) = (a.re b.re + a.im b.im, a.im b.re - a.re b.im), a b =
 * (a.re b.re - a.im b.im, a.re b.im + a.im b.re), products in the order written; the passes of the transforms over the view's
 * radix sequence, the last scaling by float32(1 / M); re re + im im.  Profile: row q of the rows_per_workgroup rows sums its
 * terms q, q + rows_per_workgroup, .. in ascending order from 0, the rows are added in ascending row order.  Estimate: the
 * block sum from 0 in ascending n, times float32(1 / Q); the residual subtracts the ports in ascending i; thread t < 256 adds
 * |e|^2 (and |y|^2) of n = t, t + 256, .. over (s, c) in ascending order, a butterfly of lane exchanges (32, 16, .., 1) per
 * wave, the four waves as (w0 + w1) + (w2 + w3), times the float32 reciprocal of the count; h_wb from 0 over (s, j), times
 * float32(1 / (n_symb n_blocks)).  An (item, receive port)'s outputs depend on nothing else: a NaN stays inside its (b, r).
 *
 *  y        complex64, row (b, r, symbol) at b item_stride + r port_stride + symbol symbol_stride, strides in complex
 *           elements, any values >= 0; 8-byte aligned, read with 8-byte loads.  Only the used combs' elements are read.
 *  slot, n_id, delay   device int32, one per item at the given element stride >= 0 (0: one value for the batch), taken as
 *           unsigned (slot mod slots_per_frame, n_id mod 30 and the low 31 bits, delay mod N): they cannot address memory
 *  profile  float32 [B][R][win_len];  h_sb complex64 [B][R][n_ap][n_symb][n_blocks];  h_wb complex64 [B][R][n_ap];  noise,
 *           epre float32 [B][R]: dense, every element written exactly once
 * One launch each on `stream`, asynchronous; n_items == 0 launches nothing.  One 256-thread workgroup per (item, receive
 * port); no atomics, no scratch, nothing read by the host.
 * CE_ERR_INVALID: abi_version != CE_ABI_VERSION; a plan value outside the ranges above; a null plan or pointer; n_items < 0;
 * n_rx outside 1..64; a negative stride or an extent beyond the address space; y not 8-byte aligned; slot, n_id, delay, profile,
 * noise, epre not 4-byte or h_sb, h_wb not 8-byte aligned.  CE_ERR_UNSUPPORTED: M = 12 or 24 without phi; more than 2^31 - 1
 * workgroups.  Nothing is written on refusal.
 */
typedef struct ce_srs_plan ce_srs_plan; /* opaque */

/* Host only: validation and derivation of ce_srs_plan_create without touching a GPU.  Every output may be NULL:
 * view of the N-point transform; info[10] = M, Q, n_blocks, n_combs, form (CE_DMRS_LP_FORM_*), N_ZC (0: table form), g, the
 * default win_len, n_words (per row of the hopping table), v_live; port_comb[4], port_cs[4]; q[30][2] and tri[M] (zero in the
 * table form); hop_words [32][n_words] (row 0: c for c_init = 0, row 1 + i: what bit i of c_init adds). */
int ce_srs_derive_host(int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs, int32_t n_symb, int32_t l0,
                       const int32_t* start_prb, int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot, int32_t hopping,
                       int32_t slots_per_frame, int32_t n_fft, int32_t win_len, const int8_t* phi, ce_tp_host_view* view,
                       int32_t* info, int32_t* port_comb, int32_t* port_cs, int32_t* q, int32_t* tri, uint32_t* hop_words);

/* Host only: the plan's tables as (re, im) float32 pairs, each optional (NULL): the N twiddles W_N[e] = exp(+j 2 pi e / N),
 * the gather table (N_ZC values W[e] = exp(-j 2 pi e / N_ZC), or the four values of the table form) and rho [n_ap][n_cs_max]. */
int ce_srs_copy_tables(int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs, int32_t n_fft, float* twiddles,
                       float* w_zc, float* rho);

/* Validates the values and uploads the tables to `device`; abi_version = CE_ABI_VERSION. */
int ce_srs_plan_create(int32_t abi_version, int32_t device, int32_t k_tc, int32_t n_ap, int32_t n_cs, int32_t k_bar, int32_t m_srs,
                       int32_t n_symb, int32_t l0, const int32_t* start_prb, int32_t n_prb_grid, int32_t n_sym, int32_t n_symb_slot,
                       int32_t hopping, int32_t slots_per_frame, int32_t n_fft, int32_t win_len, const int8_t* phi, ce_srs_plan** out);
void ce_srs_plan_destroy(ce_srs_plan* plan);

int ce_srs_profile(const ce_srs_plan* plan, const void* y, int64_t item_stride, int64_t port_stride, int64_t symbol_stride,
                   int64_t n_items, int32_t n_rx, const int32_t* slot, int64_t slot_stride, const int32_t* n_id, int64_t n_id_stride,
                   float* profile, void* stream);

int ce_srs_estimate(const ce_srs_plan* plan, const void* y, int64_t item_stride, int64_t port_stride, int64_t symbol_stride,
                    int64_t n_items, int32_t n_rx, const int32_t* slot, int64_t slot_stride, const int32_t* n_id, int64_t n_id_stride,
                    const int32_t* delay /* may be NULL */, int64_t delay_stride, void* h_sb, void* h_wb, float* noise, float* epre,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_TP_H */
