// Host-callable launchers of the HIP kernels in k_pointwise.hip, k_sos.hip, k_resample.hip and kernels2.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "sigops_internal.h"

namespace so {
// Opcodes of the expression-program operations (include/sigops.h so_eop_t) in the fused pointwise programs, next to
// sigops_internal.h's OpCode; arg = the so_un_t / so_bin_t / so_cmp_t function id (OP_INTERP: a leaf).  Only k_pointwise's math
// instantiation (launch_pointwise(..., math = true)) and the hipRTC kernels execute them.
enum MathOpCode : int32_t {
    OP_UN = 13,     // x -> f(x)
    OP_BIN = 14,    // a, b -> f(a, b)
    OP_CMP = 15,    // a, b -> (a f b) ? 1 : 0
    OP_SELECT = 16, // c, a, b -> c != 0 ? a : b
    OP_INTERP = 17  // x -> np.interp(x, table); arg = the leaf whose `base` is the table in device memory (kmath.h so_interp)
};
void launch_pointwise(const DPiece* d_pieces, int npieces, int64_t nblocks, const DOp* d_ops,
                      const DLeaf* d_leaves, OutView out, bool deep, hipStream_t st, bool chain = false, bool il = false,
                      bool math = false);
// the math instantiation (k_pointwise_math.hip, compiled with -ffp-contract=off); launch_pointwise(..., math = true) calls it
void launch_pointwise_math(const DPiece* d_pieces, int npieces, int64_t nblocks, const DOp* d_ops, const DLeaf* d_leaves,
                           OutView out, hipStream_t st);
// Counter-based noise over frame ranges (k_randn_fill.hip, -ffp-contract=off).  A piece of such a step has no programs
// (frame_len = samp_len = 0: neither the interpreter nor Plan::plan_lanes reads the op table for it), and three of the
// fields the programs would use carry its operands instead -- read and written through these names only:
constexpr int32_t& fill_noise_leaf(DPiece& p) { return p.frame_pc; }              // index of the noise leaf
constexpr int32_t fill_noise_leaf(const DPiece& p) { return p.frame_pc; }
constexpr int32_t& fill_scale_leaf(DPiece& p) { return p.samp_pc; }               // leaf of a constant factor, or -1
constexpr int32_t fill_scale_leaf(const DPiece& p) { return p.samp_pc; }
constexpr int32_t& fill_flags(DPiece& p) { return p.chain; }                      // kFillRound*
constexpr int32_t fill_flags(const DPiece& p) { return p.chain; }
constexpr int kFillRoundNoise = 1, kFillRoundProduct = 2;  // round the noise / the product to Float32 (Julia Float32 arithmetic)
// nblk_f = workgroups of kBlock Box-Muller pairs; the value goes to every channel [c0, c1) of the piece.
// The noise leaf itself (SO_FN_RANDN) keeps the seed in DLeaf::modn and the stream in DLeaf::fstride, fields a generator
// has no other use for; krand.h reads them back (randn_seed / randn_stream).
constexpr void set_randn_leaf(DLeaf& L, uint64_t seed, uint64_t stream) {
    L.modn = (int64_t)seed;
    L.fstride = (int64_t)stream;
}
void launch_randn_fill(const DPiece* d_pieces, int npieces, int64_t nblocks, const DLeaf* d_leaves, OutView out, hipStream_t st);
// returns number of kernel launches
int launch_sos_poison(void* y, const SosGeom& g, hipStream_t st);
int launch_fill_u32(void* p, size_t n, uint32_t v, hipStream_t st);  // (returns the launch's hipError_t)  // (instead of hipMemsetAsync: see k_sos.hip)
int launch_sos_poison_batch(const SosDesc* desc, int n, int dtype, hipStream_t st);
int launch_sos_batch(const SosDesc* desc, int n, int nsec, int dtype, const int64_t* total, hipStream_t st);
int launch_sos(const void* x, void* y, double* v, double* s0, const double* mpow,
               const SosGeom& g, const SosCoefs& cf, hipStream_t st);
// one pass of the three-pass IIR on its own: phase 1 (chunk end states from zero state -> v) or
// phase 3 (outputs from the chunk start states s0)
int launch_sos_phase(const void* x, void* y, double* v, const double* s0, const SosGeom& g, const SosCoefs& cf, int phase,
                     hipStream_t st);
// exact scan between them (kernels2.hip): s0[k+1] = M s0[k] + v[k] over ALL earlier chunks, no 2^-70 cut;
// mats = [M = A^L][MB = M^kXsBlock] (D x D each, row-major), sblk = [nch][nblocks][16] scratch.  3 launches.
constexpr int kXsBlock = 64;
int launch_sos_xscan(const double* v, double* s0, const double* mats, double* sblk, const SosGeom& g, int nsec, hipStream_t st);
// SOS IIR in the reference's order of operations, one sequence per channel (kernels2.hip); a: sections
// 1..8, b: sections 9..16 (b.nsec == 0: none).  0 when launched, -1: no instantiation
int launch_sos_exact(const void* x, void* y, const SosGeom& g, const SosCoefs& a, const SosCoefs& b, hipStream_t st);
// SOS IIR whose state pass was done by the resampler in front (vper: [nch][nper][16])
int launch_sos_prestate(const void* x, void* y, const double* vper, int64_t nper, const double* qmat, int pt,
                        double* v, double* s0, const double* mpow, const SosGeom& g, const SosCoefs& cf,
                        hipStream_t st);
// single-pass SOS IIR (the caller zeroes `sync` on the stream before every launch)
void launch_sos_onepass(const void* x, void* y, const SosOne& g, const SosCoefs& cf, const double* tabs,
                        int* sync, double* vpub, int dtype, hipStream_t st);
// NaN behind the first tile of a channel whose published end state (vpub, after launch_sos_onepass) is non-finite
int launch_sos_poison_onepass(void* y, const double* vpub, int nsec, const SosOne& g, int dtype, hipStream_t st);
void launch_resample(const void* x, void* y, const double* pfb, const double* dpfb,
                     const RsGeom& g, hipStream_t st);
// pfbt / dpfbt: polyphase tables transposed to [taps][nphi]
size_t resample_arb_lds_bytes(int taps, int zrows, int ct, int ringf, int esz);
int launch_resample_arb(const void* x, void* y, const double* pfbt, const double* dpfbt, const RsArb& a, hipStream_t st);
void launch_resample_tiled2(const void* x, void* y, const double* pfbt, const double* dpfbt, const RsTiled& g, hipStream_t st);
void launch_resample_tiled(const void* x, void* y, const double* pfbt, const double* dpfbt, const RsTiled& g,
                           hipStream_t st);
// returns 0 when launched, -1 when no instantiation fits the geometry
int launch_resample_rows(const void* x, void* y, const double* ctab, const int* jr, const double* mtab,
                         const int* jend, const RsRows& g, int dtype, hipStream_t st);
int launch_resample_periodic(void* y, const double* tab, const int* jend, const RsPeriodic& g,
                             int dtype, const RsGlobalTables& gsrc, hipStream_t st);
void launch_resample_fix(const RsFixArgs& a, hipStream_t st);
// fused periodic resampler -> SOS IIR (k_rsos.hip): 0 when launched, -1 when no instantiation fits
int launch_rsos_fixup(const RsFixup& fx, hipStream_t st);  // k_exact.hip
int launch_rs_fixup(const RsPerFixup& fx, hipStream_t st);   // k_exact.hip
int launch_rsos_batch(const RsosItem* items, int nitems, int gpm, const RsSos& g0, hipStream_t st);
int launch_rsos_fixup_batch(const RsFixup* items, int nitems, int nch, int out_f32, hipStream_t st);  // k_exact.hip
int launch_rsos(const double* tab, const int* jend, const RsSos& g, void* y, const RsGlobalTables& gsrc, int grid, hipStream_t st);
size_t rsos_lds_bytes(int ngroups, int ks, int rpitch, int nwaves, int cyc);
size_t rsos_lds_budget();
void launch_rms(const void* x, int dtype, int64_t n, int nch, int64_t pitch, double* partial,
                int nparts, double* rms, hipStream_t st, const RmsPatch& patch = RmsPatch{});
// SampleAt (k_sample_at.hip, -ffp-contract=off): y[i, c] = the table x read at pos[i, c] (+ base + i where `relative`),
// i in [0, n) the frames of the stage's buffer, base the absolute frame of i = 0.  Strides in elements; pcs = 0: one row of
// positions for every channel.  Returns the number of launches, -1 when the shape cannot be launched.
struct SampleAtArgs {
    const void* x;      // the table: N frames, element (j, c) at x[j * xfs + c * xcs]
    int64_t xfs, xcs, N;
    const double* pos;  // pos[i + c * pcs]
    int64_t pcs;
    double* y;          // y[i + c * ycs]
    int64_t ycs;
    int64_t base, n;
    double left, right;
    int32_t nch, x_f32, relative, wrap;
};
int launch_sample_at(const SampleAtArgs& a, hipStream_t st);
// SampleAt's cubic and windowed-sinc reads (k_sample_at_fir.hip, -ffp-contract=off): the same rows, strides and modes;
// kind 1 = Catmull-Rom, 2 = K taps of the 512-phase table `tab` (the 513 rows h, then the 512 rows dh, K doubles each, in
// device memory).  Returns the number of launches, -1 when the shape cannot be launched.
constexpr int kSampleAtPhases = 512;
struct SampleAtFirArgs {
    SampleAtArgs a;
    const double* tab;
    int32_t kind, K;
};
int launch_sample_at_fir(const SampleAtFirArgs& f, hipStream_t st);
bool sample_at_fir_uses_lds(const SampleAtFirArgs& f);  // (the sinc kernel's form with the tap table in LDS: K <= 16, a large result)
// Comb / Allpass (k_comb.hip, -ffp-contract=off): per channel y[n] = (b0 * x[n] + bD * x[n - D]) + a * y[n - D], n in [0, n),
// x and y before frame 0 taken as +0.0, every product and sum rounded on its own; a term whose coefficient is exactly 0.0
// is left out.  One lane per (residue n mod D, channel) walks its class in order.  Strides in elements.  Returns the
// number of launches, -1 when the shape cannot be launched.
constexpr int kCombUnroll = 16;  // steps of a lane whose loads are issued before the arithmetic that depends on them
struct CombArgs {
    const void* x;  // element (n, c) at x[n * xfs + c * xcs]
    int64_t xfs, xcs;
    double* y;      // y[n + c * ycs]
    int64_t ycs;
    int64_t n, D;
    double b0, bD, a;
    int32_t nch, x_f32;
    // The resumed form (a stream's push, DESIGN.md "Streaming the device-only nodes"): frame 0 of x and y is frame r of the
    // signal, and the lane of residue class (r + j) mod D takes its (xd, yd) from the record instead of +0.0 and leaves the
    // pair it ends with in the other record.  A record is [nch][D][2] Float64; a class without a frame in [r, r + n) copies
    // its entry.  cin is read only where r > 0; cout may be null.  All three zero: the kernel of a whole signal, as ever.
    int64_t r;
    const double* cin;
    double* cout;
};
int launch_comb(const CombArgs& a, hipStream_t st);
// Cumsum (k_cumsum.hip, -ffp-contract=off): per channel y[n] = x[0] + ... + x[n] in Float64 over ONE summation tree that
// depends on the frame index only (DESIGN.md "Cumsum"): runs of kCumsumRun frames summed left to right, an inclusive
// Kogge-Stone scan over the 64 run totals of a tile, a sequential carry over the kCumsumTiles tiles of a chunk and a
// sequential carry over the chunks.  Reduce-then-scan, no workgroup waits for another: k_cumsum_totals (the chunk-local
// last value of every chunk but the last -> tot), k_cumsum_carry (tot -> the running sum of tot, in place, one workgroup
// per channel), k_cumsum_scan (recomputes the chunk, adds the carry, stores).  A signal of one chunk is one launch.
// Strides in elements.  Returns the number of launches, -1 when the shape cannot be launched.
constexpr int kCumsumRun = 16;    // L: frames a lane sums left to right
constexpr int kCumsumTiles = 16;  // G: tiles (64 runs each) a workgroup carries through sequentially
constexpr int kCumsumTile = 64 * kCumsumRun, kCumsumChunk = kCumsumTile * kCumsumTiles;
struct CumsumArgs {
    const void* x;  // element (n, c) at x[n * xfs + c * xcs]
    int64_t xfs, xcs;
    double* y;      // y[n + c * ycs]
    int64_t ycs;
    double* tot;    // [nch][tot_pitch] scratch, tot_pitch >= cumsum_totals(n)
    int64_t tot_pitch;
    int64_t n;
    int32_t nch, x_f32;
    // The resumed form (a stream's push): frame 0 of x and y is frame k0 * kCumsumChunk of the signal, cin[c] the running
    // total that enters that chunk (read only where k0 > 0).  cout[c], where it is not null and n covers more than one
    // chunk, receives the total that enters the LAST chunk of [0, n): what a later launch resumes from.
    int64_t k0;
    const double* cin;
    double* cout;
};
// the chunk totals a channel of n frames needs: one for every chunk that has a chunk behind it
constexpr int64_t cumsum_totals(int64_t n) { return n <= kCumsumChunk ? 0 : (n - 1) / kCumsumChunk; }
int launch_cumsum(const CumsumArgs& a, hipStream_t st);
// Recur / OnePole / Smooth / PeakDecay (k_recur.hip, -ffp-contract=off): per channel the first-order scan
// y[n] = J(a[n], y[n-1], b[n]), y[0] = b[0], in Float64 over Cumsum's tree (the constants above; DESIGN.md "Recur";
// tests/recur_ref.py is the definition).  J(a, v, w) with m = a * v rounded once: op 0 m + w (never an FMA), op 1 the
// greater of m and w, NaN if either is.  An element of the scan is a pair (product of a, value); runs of kCumsumRun frames
// left to right, a Kogge-Stone scan over the 64 run totals of a tile, sequential carries over the kCumsumTiles tiles of a
// chunk and over the chunks.  Reduce-then-scan, no workgroup waits for another: k_recur_totals (the chunk-local last pair
// of every chunk but the last -> tot), k_recur_carry (tot -> the carry C behind every chunk, in place, one workgroup per
// channel), k_recur_scan (recomputes the chunk, applies C, stores).  A signal of one chunk is one launch.  Strides in
// elements.  Returns the number of launches, -1 when the shape cannot be launched.
struct RecurArgs {
    const void* b;    // element (n, c) at b[n * bfs + c * bcs]
    int64_t bfs, bcs;
    const double* a;  // a row of coefficients per channel, a[n + c * acs] (acs 0: one row for every channel); nullptr: the constant ac
    int64_t acs;
    double ac;
    double* y;        // y[n + c * ycs]
    int64_t ycs;
    double* tot;      // [nch][tot_pitch][2] scratch, tot_pitch >= cumsum_totals(n): (Q[last], u[last]) of a chunk, then (Q[last], C)
    int64_t tot_pitch;
    int64_t n;
    int32_t nch, b_f32, op;
    // the resumed form, as CumsumArgs': the state is the carry C, one Float64 a channel
    int64_t k0;
    const double* cin;
    double* cout;
};
int launch_recur(const RecurArgs& a, hipStream_t st);
// Recur2 / Resonator / Sweep (k_recur2.hip, -ffp-contract=off): per channel the second-order scan
// y[n] = (a1[n] y[n-1] + a2[n] y[n-2]) + b[n], y[0] = b[0], y[1] = (a1[1] y[0] + a2[1] (+0.0)) + b[1], in Float64 over
// Cumsum's tree (the constants above; DESIGN.md "Recur2"; tests/recur2_ref.py is the definition), every product and every
// sum rounded on its own.  An element of the scan is (M, v), the affine map s -> M s + v on the state s = (y[n], y[n-1]):
// six entries.  Inside a run of kCumsumRun frames the composite advances by a shift in Float64 (row 0 <- a1 row 0 + a2
// row 1, row 1 <- the old row 0); the 64 run totals of a tile go through a Kogge-Stone scan of joins whose entries are
// double-doubles (error-free transformations in plain Float64 operations, no FMA); a state is carried from tile to tile
// of a chunk, a composite and then a state from chunk to chunk; the outputs of a run are the recurrence itself walked
// from the state that entered it.
// Reduce-then-scan, no workgroup waits for another: k_recur2_totals (the chunk-local composite of every chunk but the last
// -> tot), k_recur2_carry (tot -> the state that enters the chunk behind, in place of the composite's v, one workgroup per
// channel), k_recur2_scan (recomputes the chunk, applies the entering state, stores).  A signal of one chunk is one
// launch.  Strides in elements.  Returns the number of launches, -1 when the shape cannot be launched.
struct Recur2Args {
    const void* b;     // element (n, c) at b[n * bfs + c * bcs]
    int64_t bfs, bcs;
    const double* a[2];  // a1, a2: a row of coefficients per channel, a[i][n + c * acs[i]] (acs 0: one row for every channel); both nullptr: the constants ac
    int64_t acs[2];
    double ac[2];
    double* y;         // y[n + c * ycs]
    int64_t ycs;
    double* tot;       // [nch][tot_pitch][12] scratch, tot_pitch >= cumsum_totals(n): the high words (M00, M01, M10, M11, v0, v1) of a chunk, then the low words; v0, v1 become (s0, s1)
    int64_t tot_pitch;
    int64_t n;
    int32_t nch, b_f32;
    // the resumed form, as CumsumArgs': the state is (s0, s1) as k_recur2_carry leaves it -- the chunk's composite applied in
    // double-double arithmetic, NOT the last two outputs, whose bits differ -- two Float64 a channel
    int64_t k0;
    const double* cin;
    double* cout;
};
int launch_recur2(const Recur2Args& a, hipStream_t st);
// MovingMax / MovingMin (k_moving.hip): output j in [0, n_out) of a channel is the greatest (least) of the input frames
// [j + off - back, j + off + ahead] clipped to [0, n_in), under the order -Inf < .. < -0.0 < +0.0 < .. < +Inf, NaN if any of
// them is NaN; the result has the input's type and is a bit copy of that sample.  Compared on a monotone integer key, so any
// split of the work gives the same bits (DESIGN.md "Moving extrema").  A window of at most kMovHalo + 1 frames is one
// launch (k_moving_short: tile + halo in LDS, a suffix and a prefix scan over power-of-two segments); a longer one is 2 + levels launches
// (k_moving_blockmax: the maximum of every aligned block of kMovTile input frames; k_moving_level: a sparse table over
// them; k_moving_long: in-block suffix, two table look-ups, in-block prefix).  No workgroup waits for another, no atomics.
// Strides in elements.  Returns the number of launches, -1 when the shape cannot be launched.
constexpr int kMovTile = 2048;  // T: output frames of a workgroup; input frames of a block of the long form (a power of two)
constexpr int kMovHalo = 2048;  // H: the short form takes W - 1 <= H (H >= T - 1: a longer window never lies inside one block)
struct MovingArgs {
    const void* x;  // input frame i, channel c at x[i * xfs + c * xcs], i in [0, n_in)
    int64_t xfs, xcs, n_in;
    void* y;        // y[j + c * ycs], j in [0, n_out), of the input's type
    int64_t ycs, n_out;
    int64_t off;    // the input frame output 0 is centred on (0 <= off, off + n_out <= n_in)
    int64_t back, ahead;
    void* tab;      // long form: [levels + 1][nch][nblocks] keys of 8 bytes (moving_scratch); unused by the short form
    int32_t nch, f32, is_min;
};
// the long form's table: its levels above the block maxima, and its entries (of 8 bytes) a channel; 0 for the short form
constexpr int64_t moving_clamp(int64_t v, int64_t n_in) { return v < n_in ? v : n_in; }
constexpr bool moving_is_long(int64_t n_in, int64_t back, int64_t ahead) { return moving_clamp(back, n_in) + moving_clamp(ahead, n_in) > kMovHalo; }
constexpr int64_t moving_blocks(int64_t n_in) { return (n_in + kMovTile - 1) / kMovTile; }
constexpr int moving_levels(int64_t n_in, int64_t back, int64_t ahead) {
    // a window holds at most (W - 1) / T whole blocks between the two it starts and ends in
    int64_t mid = (moving_clamp(back, n_in) + moving_clamp(ahead, n_in)) / kMovTile;
    if (mid > moving_blocks(n_in)) mid = moving_blocks(n_in);
    int l = 0;
    while (((int64_t)2 << l) <= mid) ++l;
    return l;
}
constexpr int64_t moving_scratch(int64_t n_in, int64_t back, int64_t ahead) {
    return moving_is_long(n_in, back, ahead) ? (int64_t)(moving_levels(n_in, back, ahead) + 1) * moving_blocks(n_in) : 0;
}
int launch_moving(const MovingArgs& a, hipStream_t st);
// MovingSum / MovingMean / MovingRMS (k_movsum.hip, -ffp-contract=off): output j in [0, n_out) of a channel is the Float64
// sum of the input frames [j + off - back, j + off + ahead] clipped to [0, n_in) (rms: of their squares), over ONE summation
// tree fixed by the ABSOLUTE frame numbers of x -- input frame i is frame abs0 + i of x -- and by back and ahead alone
// (DESIGN.md "Moving sums"; tests/movingsum_ref.py): what lies outside the signal is -0.0, the additive identity; segments
// [m S, (m + 1) S) of S = min(kMsumBlock, the greatest power of two <= W - 1) frames; inside one, runs of kMsumRun frames summed
// left to right (right to left) and an inclusive Kogge-Stone scan over the run totals give the prefix P and the suffix Q; the
// window is (Q(lo) + M) + P(hi), M the whole segments in between.  W - 1 <= kMsumHalo is one launch (k_movsum_short: the tile,
// its halo and the lead-in to a multiple of S in LDS, M one segment's total at most); a longer window has S = kMsumBlock and
// is 2 + levels launches (k_movsum_totals: the total of every aligned block; k_movsum_level: the aligned dyadic nodes over
// them, node (l, q) = node (l - 1, 2 q) + node (l - 1, 2 q + 1); k_movsum_long: Q and P from the blocks the tile's windows
// start and end in, M the canonical cover of the blocks in between by maximal aligned nodes, added left to right).  The
// mean divides by the frames of the clipped window, the rms takes the square root of that quotient.  No workgroup waits
// for another, no atomics.  Strides in elements.  Returns the number of launches, -1 when the shape cannot be launched.
constexpr int kMsumRun = 16;      // R: frames of a run
constexpr int kMsumBlock = 1024;  // B: the longest segment; a block of the long form
constexpr int kMsumTile = 2048;   // output frames of a workgroup
constexpr int kMsumHalo = 1024;   // the short form takes W - 1 <= this: its image holds kMsumTile + kMsumHalo + (S - 1) <= 4095 keys
struct MovsumArgs {
    const void* x;  // input frame i, channel c at x[i * xfs + c * xcs], i in [0, n_in)
    int64_t xfs, xcs, n_in;
    double* y;      // y[j + c * ycs], j in [0, n_out)
    int64_t ycs, n_out;
    int64_t off;    // the input frame output 0 is centred on (0 <= off, off + n_out <= n_in)
    int64_t abs0;   // the frame of x that input frame 0 is (>= 0; the windows reach no frame of x in [0, abs0))
    int64_t back, ahead;
    double* tab;    // long form: [levels + 1][nch][nblocks] Float64 (movsum_scratch); unused by the short form
    int32_t nch, x_f32;
    int32_t op;     // 0 sum, 1 mean, 2 rms
};
constexpr bool movsum_is_long(int64_t back, int64_t ahead) { return back > kMsumHalo || ahead > kMsumHalo || back + ahead > kMsumHalo; }
// the aligned blocks of x that hold the input frames [abs0, abs0 + n_in), n_in >= 1
constexpr int64_t movsum_blocks(int64_t abs0, int64_t n_in) { return (abs0 + n_in - 1) / kMsumBlock - abs0 / kMsumBlock + 1; }
// the levels above the block totals: a cover lies inside the (W - 1) / B whole blocks a window can hold, and a node of
// more than `blocks` blocks that starts inside them equals its leftmost node of ceil(log2(blocks)) levels (the rest is -0.0)
constexpr int movsum_levels(int64_t abs0, int64_t n_in, int64_t back, int64_t ahead) {
    const int64_t cap = (int64_t)1 << 60;
    const int64_t reach = (back < cap ? back : cap) + (ahead < cap ? ahead : cap);
    const int64_t mid = reach / kMsumBlock, nb = movsum_blocks(abs0, n_in);
    int l = 0;
    while (((int64_t)2 << l) <= mid && ((int64_t)1 << l) < nb) ++l;
    return l;
}
constexpr int64_t movsum_scratch(int64_t abs0, int64_t n_in, int64_t back, int64_t ahead) {
    return movsum_is_long(back, ahead) ? (int64_t)(movsum_levels(abs0, n_in, back, ahead) + 1) * movsum_blocks(abs0, n_in) : 0;
}
int launch_movsum(const MovsumArgs& a, hipStream_t st);
// MovingMedian / MovingQuantile (k_movrank.hip, -ffp-contract=off): output j in [0, n_out) of a channel is a bit copy of the
// sample of rank floor(q (m - 1)), counted from 0, among the m input frames [j + off - back, j + off + ahead] clipped to
// [0, n_in), under the order -Inf < .. < -0.0 < +0.0 < .. < +Inf (k_moving.hip's integer key); NaN if any of them is NaN; the
// result has the input's type (DESIGN.md "Moving ranks"; tests/movingmedian_ref.py).  ONE form, one launch (k_movrank): a tile
// of kRankTile outputs and its halo in LDS, every element of the image counts its own rank in the first window that holds
// it and updates it from window to window; the element whose rank is the target writes its index.  Takes
// min(back, n_in) + min(ahead, n_in) <= kRankHalo.  No workgroup waits for another, no atomics.  Strides in elements.
// Returns the number of launches, -1 when the shape cannot be launched (a longer window among them).
constexpr int kRankTile = 2048;  // T: output frames of a workgroup
constexpr int kRankHalo = 1024;  // H: W - 1 <= H; the image holds T + 3 H keys (the tile, its halo and a guard of W - 1 keys on either side)
struct MovrankArgs {
    const void* x;  // input frame i, channel c at x[i * xfs + c * xcs], i in [0, n_in)
    int64_t xfs, xcs, n_in;
    void* y;        // y[j + c * ycs], j in [0, n_out), of the input's type
    int64_t ycs, n_out;
    int64_t off;    // the input frame output 0 is centred on (0 <= off, off + n_out <= n_in)
    int64_t back, ahead;
    double q;       // in [0, 1]
    int32_t nch, f32;
};
constexpr bool movrank_fits(int64_t n_in, int64_t back, int64_t ahead) { return moving_clamp(back, n_in) + moving_clamp(ahead, n_in) <= kRankHalo; }
int launch_movrank(const MovrankArgs& a, hipStream_t st);
}  // namespace so
