// DSP.jl phase accumulator replay for the arbitrary-rate resampler (see the comment below) and the
// host-only position diagnostics of the C-ABI (so_resample_positions).
#include <chrono>
#include <thread>
#include <string>
#include <unistd.h>

#include "plan_impl.h"

namespace so {

// ---------------------------------------------------------------------------
// DSP.jl FIRArbitrary positions (reference call sites
// src/reformatting.jl:92-98 `setphase!(self, timedelay(self))`, src/filters.jl:252-255 `filt!`):
//     ϕAcc += Δ;  if ϕAcc > Nϕ:  xIdx += div(ϕAcc-1, Nϕ);  ϕAcc = mod(ϕAcc-1, Nϕ) + 1
//     ϕIdx = floor(ϕAcc);  α = ϕAcc - ϕIdx
// once per output, in Float64.  The sequence is data independent and does not depend on the
// block size (xIdx is carried as inputDeficit), so it is replayed here once per plan and compared
// with the kernels' closed-form rule.  At a tie (closed-form α == 0) accumulated rounding error
// leaves the accumulator a hair below the integer: (previous phase, α ≈ 1).  The interpolated
// taps h + α·dh are continuous there EXCEPT (a) across the wrap (ϕIdx = Nϕ, α ≈ 1, xIdx not
// advanced: the tap h[0] of the next input is dropped) and (b) at the filter's last tap
// (dh = [diff(h); 0] ends in 0, not -h[end]) -- differences of ~1e-3 of a sample.  For a rational
// pattern (integer frame rates) both happen at the same place of (nearly) every period:
// `prev[r]` marks those period positions so that the kernels' tap tables are built with the
// accumulator's (fine position - 1, α = 1) there; every other deviation that changes the taps
// goes to the fix-up list (k_resample_fix).
static void replay_phase_accumulator_impl(const RsGeom& g, const double* h, int hlen, int64_t from, int64_t need, bool bake,
                                          std::vector<uint8_t>& prev, std::vector<RsFix>& fix);

// state of the accumulator before output m (a later window of the same resampler resumes from the
// nearest one instead of replaying from output 0)
struct AccCheckpoint {
    int64_t m, xb;
    double acc;
};
static uint64_t taps_fnv(const double* h, int hlen) {  // (hsum alone, a weighted sum, collides for permuted or compensating taps)
    uint64_t f = 1469598103934665603ull;
    const unsigned char* hb = reinterpret_cast<const unsigned char*>(h);
    for (size_t i = 0; i < (size_t)hlen * sizeof(double); ++i) f = (f ^ hb[i]) * 1099511628211ull;
    return f;
}
struct AccKey {
    double delta, c0, hsum;
    uint64_t hfnv;  // FNV-1a over the taps' bytes
    int64_t c0i, L, M;
    int32_t nphi, taps, exact, hlen;
    bool operator==(const AccKey& o) const { return std::memcmp(this, &o, sizeof(AccKey)) == 0; }
};
static std::mutex g_acc_mu;
static std::vector<std::pair<AccKey, std::vector<AccCheckpoint>>> g_acc_checkpoints;
static AccKey acc_key(const RsGeom& g, const double* h, int hlen) {
    AccKey k;
    std::memset(&k, 0, sizeof k);
    k.delta = g.delta;
    k.c0 = g.c0;
    k.c0i = g.c0i;
    k.L = g.L;
    k.M = g.M;
    k.nphi = g.nphi;
    k.taps = g.taps;
    k.exact = g.exact;
    k.hlen = hlen;
    for (int i = 0; i < hlen; ++i) k.hsum += h[i] * (1.0 + 1e-3 * (i % 97));
    k.hfnv = taps_fnv(h, hlen);
    return k;
}

// The replay is sequential by nature (~5 ns per output: 160 ms for config 3's 28.8 M outputs) and
// depends only on the geometry, so a process keeps the last few results (plans of the same
// resampler -- a bench's second workload, a re-created plan -- get it for free).
// Outputs [from, need) (absolute); `from` is a whole number of periods of an exact rational rate (any output of a rate
// without a period), and the fix-up list comes back in the window's own coordinates (output m - from, input
// j - from/L*M, or j - g.j0).
// Version of everything a cached replay or probe value depends on besides its key: the replay itself, RsFix and how the
// fix-up list is generated, the cascade's sensitivity probes.  Part of the key (and so of the file name and of the
// header that is compared byte for byte): a build that changes any of them bumps it, and the files of older builds are
// simply never looked at again.
constexpr int32_t kAccAlgoVersion = 7;  // (7: the chunked-form probe sees state-matrix powers rounded once, stages.cpp matpow)

void replay_phase_accumulator(const RsGeom& g, const double* h, int hlen, int64_t need, bool bake,
                                     std::vector<uint8_t>& prev, std::vector<RsFix>& fix, int64_t from) {
    struct Key {
        double delta, c0, hsum;
        uint64_t hfnv;  // FNV-1a over the taps' bytes (hsum alone, a weighted sum, collides for permuted or compensating taps)
        int64_t c0i, L, M, need, from, j0;
        int32_t nphi, taps, exact, hlen, bake;
        int32_t version;  // kAccAlgoVersion: what a file was computed WITH, not only FOR
        bool operator==(const Key& o) const { return std::memcmp(this, &o, sizeof(Key)) == 0; }
    };
    struct Entry {
        Key k;
        std::vector<uint8_t> prev;
        std::vector<RsFix> fix;
    };
    static std::mutex mu;
    static std::vector<Entry> cache;
    Key k;
    std::memset(&k, 0, sizeof k);
    k.delta = g.delta;
    k.c0 = g.c0;
    k.c0i = g.c0i;
    k.L = g.L;
    k.M = g.M;
    k.need = need;
    k.from = from;
    k.j0 = g.j0;
    k.nphi = g.nphi;
    k.taps = g.taps;
    k.exact = g.exact;
    k.hlen = hlen;
    k.bake = bake;
    for (int i = 0; i < hlen; ++i) k.hsum += h[i] * (1.0 + 1e-3 * (i % 97));
    k.hfnv = taps_fnv(h, hlen);
    k.version = kAccAlgoVersion;
    if (!g.arbitrary || need <= 0) {
        prev.clear();
        fix.clear();
        return;
    }
    const bool nocache = std::getenv("SIGOPS_REPLAY_NOCACHE") != nullptr;  // (tests: compare replays, not cache hits)
    if (!nocache) {
        std::lock_guard<std::mutex> lock(mu);
        for (auto& e : cache)
            if (e.k == k) {
                prev = e.prev;
                fix = e.fix;
                return;
            }
    }
    // ... and, where the host names a directory (SIGOPS_CACHE_DIR, as for the hipRTC code objects: a library does not write
    // under $HOME by itself), between processes: the result depends on nothing but the key -- which the file carries in
    // full and which is compared byte for byte --, and a one-shot `sink` of ten minutes of audio spends 11 of its 17
    // plan-creation milliseconds here.  Written under a per-process temporary name and renamed; a file that does not
    // check out is ignored (and overwritten by the replay's result).
    std::string path;
    if (!nocache)
        if (const char* d = std::getenv("SIGOPS_CACHE_DIR")) {
            uint64_t hsh = 1469598103934665603ull;  // FNV-1a over the key
            const unsigned char* kb = reinterpret_cast<const unsigned char*>(&k);
            for (size_t i = 0; i < sizeof k; ++i) hsh = (hsh ^ kb[i]) * 1099511628211ull;
            char nm[64];
            std::snprintf(nm, sizeof nm, "/sigops_acc_%016llx.bin", (unsigned long long)hsh);
            path = std::string(d) + nm;
            if (FILE* f = std::fopen(path.c_str(), "rb")) {
                struct Hdr {
                    uint64_t magic, nprev, nfix;
                    Key k;
                } hd;
                bool ok = std::fread(&hd, sizeof hd, 1, f) == 1 && hd.magic == 0x31636361736f6973ull && hd.k == k && hd.nprev < (1ull << 32) &&
                          hd.nfix < (1ull << 28);
                std::vector<uint8_t> pv;
                std::vector<RsFix> fx;
                if (ok) {
                    pv.resize((size_t)hd.nprev);
                    fx.resize((size_t)hd.nfix);
                    ok = (hd.nprev == 0 || std::fread(pv.data(), 1, pv.size(), f) == pv.size()) &&
                         (hd.nfix == 0 || std::fread(fx.data(), sizeof(RsFix), fx.size(), f) == fx.size()) && std::fgetc(f) == EOF;
                }
                std::fclose(f);
                if (ok) {
                    prev.swap(pv);
                    fix.swap(fx);
                    std::lock_guard<std::mutex> lock(mu);
                    if (cache.size() >= 8) cache.erase(cache.begin());
                    cache.push_back(Entry{k, prev, fix});
                    return;
                }
            }
        }
    replay_phase_accumulator_impl(g, h, hlen, from, need, bake, prev, fix);
    if (!path.empty()) {
        char tmp[64];
        std::snprintf(tmp, sizeof tmp, ".%ld.%p.tmp", (long)getpid(), (void*)&k);
        const std::string tpath = path + tmp;
        if (FILE* f = std::fopen(tpath.c_str(), "wb")) {
            struct Hdr {
                uint64_t magic, nprev, nfix;
                Key k;
            } hd;
            std::memset(&hd, 0, sizeof hd);
            hd.magic = 0x31636361736f6973ull;
            hd.nprev = prev.size();
            hd.nfix = fix.size();
            hd.k = k;
            const bool ok = std::fwrite(&hd, sizeof hd, 1, f) == 1 && (prev.empty() || std::fwrite(prev.data(), 1, prev.size(), f) == prev.size()) &&
                            (fix.empty() || std::fwrite(fix.data(), sizeof(RsFix), fix.size(), f) == fix.size());
            const bool closed = std::fclose(f) == 0;
            if (!(ok && closed && std::rename(tpath.c_str(), path.c_str()) == 0)) std::remove(tpath.c_str());
        }
    }
    std::lock_guard<std::mutex> lock(mu);
    if (cache.size() >= 8) cache.erase(cache.begin());
    cache.push_back(Entry{k, prev, fix});
}

static std::string disk_value_path(const char* kind, const std::vector<double>& key) {
    const char* d = std::getenv("SIGOPS_CACHE_DIR");
    if (!d || !*d || std::getenv("SIGOPS_REPLAY_NOCACHE")) return std::string();
    uint64_t hsh = 1469598103934665603ull;  // FNV-1a over the key
    const unsigned char* kb = reinterpret_cast<const unsigned char*>(key.data());
    for (size_t i = 0; i < key.size() * sizeof(double); ++i) hsh = (hsh ^ kb[i]) * 1099511628211ull;
    char nm[96];
    std::snprintf(nm, sizeof nm, "/sigops_%s_v%d_%016llx.bin", kind, (int)kAccAlgoVersion, (unsigned long long)hsh);
    return std::string(d) + nm;
}
bool disk_value_get(const char* kind, const std::vector<double>& key, double& val) {
    const std::string path = disk_value_path(kind, key);
    if (path.empty()) return false;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    uint64_t hd[2] = {0, 0};
    std::vector<double> k(key.size());
    double v = 0.0;
    const bool ok = std::fread(hd, sizeof hd, 1, f) == 1 && hd[0] == 0x316c6176736f6973ull && hd[1] == key.size() &&
                    (k.empty() || std::fread(k.data(), sizeof(double), k.size(), f) == k.size()) && std::fread(&v, sizeof v, 1, f) == 1 &&
                    std::fgetc(f) == EOF && std::memcmp(k.data(), key.data(), k.size() * sizeof(double)) == 0;
    std::fclose(f);
    if (ok) val = v;
    return ok;
}
void disk_value_put(const char* kind, const std::vector<double>& key, double val) {
    const std::string path = disk_value_path(kind, key);
    if (path.empty()) return;
    char tmp[64];
    std::snprintf(tmp, sizeof tmp, ".%ld.%p.tmp", (long)getpid(), (const void*)&key);
    const std::string tpath = path + tmp;
    FILE* f = std::fopen(tpath.c_str(), "wb");
    if (!f) return;
    const uint64_t hd[2] = {0x316c6176736f6973ull, (uint64_t)key.size()};
    const bool ok = std::fwrite(hd, sizeof hd, 1, f) == 1 && (key.empty() || std::fwrite(key.data(), sizeof(double), key.size(), f) == key.size()) &&
                    std::fwrite(&val, sizeof val, 1, f) == 1;
    const bool closed = std::fclose(f) == 0;
    if (!(ok && closed && std::rename(tpath.c_str(), path.c_str()) == 0)) std::remove(tpath.c_str());
}

static void replay_phase_accumulator_impl(const RsGeom& g, const double* h, int hlen, int64_t from, int64_t need, bool bake,
                                          std::vector<uint8_t>& prev, std::vector<RsFix>& fix) {
    prev.clear();
    fix.clear();
    if (!g.arbitrary || need <= 0) return;
    const auto t_r0 = std::chrono::steady_clock::now();
    auto t_r1 = t_r0, t_r2 = t_r0, t_r3 = t_r0;
    const int nphi = g.nphi, taps = g.taps;
    const double dnphi = (double)nphi;
    const bool pow2 = (nphi & (nphi - 1)) == 0;
    const double inv = 1.0 / dnphi;
    double hmax = 0.0;
    for (int i = 0; i < hlen; ++i) hmax = std::max(hmax, std::fabs(h[i]));
    auto tap = [&](int64_t q, double alpha, int64_t k) -> double {  // tap applied to input (q/nphi - k)
        if (k < 0 || k >= taps) return 0.0;
        const int64_t hi = q % nphi + (int64_t)nphi * k;
        const double hv = hi < hlen ? h[hi] : 0.0;
        const double dv = hi + 1 < hlen ? h[hi + 1] - h[hi] : 0.0;
        return hv + alpha * dv;
    };
    // do the two positions give different taps (beyond the interpolation's own continuity)?
    auto taps_differ = [&](int64_t qa, double aa, int64_t qe, double ae) {
        const int64_t ja = qa / nphi, je = qe / nphi, dj = je - ja;
        if (std::llabs(dj) > 1) return true;
        double d = 0.0;
        for (int64_t k = -1; k <= taps; ++k) d = std::max(d, std::fabs(tap(qa, aa, k) - tap(qe, ae, k + dj)));
        return d > 4e-6 * hmax;  // (positions within 1e-6 of each other move a tap by < 1e-6*|dh|)
    };
    // setphase!(kernel, τ), τ = (hLen-1)/(2Nϕ)
    const double tau = (double)(hlen - 1) / 2.0 / dnphi;
    const double w = std::floor(tau), fr = tau - w;
    int64_t xb = (int64_t)std::llround(w) * nphi;  // (xIdx-1)*Nϕ, xIdx = inputDeficit = 1 + w
    double acc = fr * dnphi + 1.0;
    const double delta = g.delta;
    // closed-form rule of the kernels
    const bool exact = g.exact != 0;
    const int64_t L = g.L, dq = exact ? ((int64_t)nphi * g.M) / L : 0, dfr = exact ? ((int64_t)nphi * g.M) % L : 0;
    struct Rec { int64_t m, qa; double alpha; };
    std::vector<Rec> rec;
    // The deviations in pieces, in output order: what ran before the threaded ranges, each confirmed range (its list moved,
    // not copied: 360 000 records for ten minutes of 44.1 -> 48 kHz), the rest.  Each piece with the counts the lists below
    // are decided by -- per period position: records, records of the baked form -- made by the thread that made the piece.
    struct Part {
        std::vector<Rec> rec;
        int64_t ma = 0, mb = 0;       // outputs [ma, mb) (records only of outputs >= from)
        std::vector<int64_t> ca, cb;  // per period position: records / of the baked form (empty: no period, or not counted)
    };
    std::vector<Part> parts;
    const bool periodic = exact && L >= 1 && L <= 65536;
    auto exact_q = [&](int64_t m) {
        const int64_t Nn = m * ((int64_t)nphi * g.M);
        return g.c0i + Nn / L;
    };
    auto baked = [&](const Rec& r) { return r.qa == exact_q(r.m) - 1 && r.alpha > 0.5; };
    auto count_part = [&](Part& pa) {
        if (!periodic) return;
        pa.ca.assign((size_t)L, 0);
        pa.cb.assign((size_t)L, 0);
        for (const Rec& r : pa.rec) {
            const size_t pos = (size_t)(r.m % L);
            pa.ca[pos]++;
            if (baked(r)) pa.cb[pos]++;
        }
    };
    int64_t m0 = 0;
    const AccKey ckey = acc_key(g, h, hlen);
    std::vector<AccCheckpoint> made;
    if (from > 0 && !std::getenv("SIGOPS_REPLAY_NOCACHE")) {  // resume from the nearest checkpoint at or before the window
        std::lock_guard<std::mutex> lock(g_acc_mu);
        for (auto& e : g_acc_checkpoints)
            if (e.first == ckey)
                for (auto& c : e.second)
                    if (c.m <= from && c.m > m0) {
                        m0 = c.m;
                        xb = c.xb;
                        acc = c.acc;
                    }
    }
    // outputs [ma, mb) from the accumulator state (xb, acc) before output ma; deviations of outputs
    // >= from are appended to `out`; the state before output mb is left in (xb, acc)
    auto run = [&](int64_t ma, int64_t mb, int64_t& xb, double& acc, std::vector<Rec>& out, std::vector<int8_t>& memo) {
        int64_t qe = g.c0i, fe = 0;
        if (exact) {
            const __int128 Nn = (__int128)ma * ((int64_t)nphi * g.M);
            qe = g.c0i + (int64_t)(Nn / L);
            fe = (int64_t)(Nn % L);
        }
        for (int64_t m = ma; m < mb; ++m) {
            const int pi = (int)acc;  // floor: acc >= 1
            const int64_t qa = xb + pi - 1;
            double qe_frac = 0.0;
            if (!exact) {
                const double t = (double)m * delta;  // two separately rounded operations, like rs_pos
                const double q = g.c0 + t;
                const double fl = std::floor(q);
                qe = (int64_t)fl;
                qe_frac = q - fl;
            }
            if (qa != qe) {
                const double alpha = acc - (double)pi;
                const double ae = exact ? (double)fe / (double)L : qe_frac;
                bool differ;
                const bool tie = exact && fe == 0 && std::llabs(qa - qe) == 1 && (alpha < 1e-6 || alpha > 1.0 - 1e-6);
                if (tie) {
                    int8_t& mm = memo[(size_t)(qe % nphi) * 4 + (qa > qe ? 2 : 0) + (alpha > 0.5 ? 1 : 0)];
                    if (mm < 0) mm = taps_differ(qa, alpha > 0.5 ? 1.0 : 0.0, qe, 0.0) ? 1 : 0;
                    differ = mm != 0;
                } else differ = taps_differ(qa, alpha, qe, ae);
                if (differ && m >= from) out.push_back(Rec{m, qa, alpha});
            }
            if (exact) {
                qe += dq;
                fe += dfr;
                if (fe >= L) {
                    fe -= L;
                    ++qe;
                }
            }
            acc += delta;
            if (acc > dnphi) {
                // xIdx += div(ϕAcc-1, Nϕ); ϕAcc = mod(ϕAcc-1, Nϕ) + 1.  (ϕAcc-1 and the remainder are
                // exact, the final +1 rounds: the same real number as ϕAcc - k·Nϕ rounded once)
                const double a1 = acc - 1.0;
                if (a1 < dnphi) {
                    // k == 0: unchanged
                } else if (a1 < 2.0 * dnphi) {
                    xb += nphi;
                    acc -= dnphi;
                } else if (pow2) {
                    const double k = std::floor(a1 * inv);
                    xb += (int64_t)k * nphi;
                    acc -= k * dnphi;
                } else {
                    const double k = std::floor(a1 / dnphi);
                    xb += (int64_t)k * nphi;
                    acc = std::fmod(a1, dnphi) + 1.0;
                }
            }
        }
    };
    std::vector<int8_t> memo0((size_t)nphi * 4, -1);  // exact ties: (phase of qe, qa-qe, α snapped) -> differ?
    made.push_back(AccCheckpoint{m0, xb, acc});
    int64_t mcur = m0;
    // ---- long replays of an exact rational rate, several threads.  The accumulator turns out to be
    //      periodic up to a constant: ϕAcc(m + L) = ϕAcc(m) + δ bit for bit (δ ~ -2e-13 for 44.1 -> 48 kHz,
    //      the same for 30 M outputs), xIdx(m + L) = xIdx(m) + M.  That PREDICTS the state before any
    //      output; every thread replays its own range from the predicted state, and the prediction is
    //      then VERIFIED: the state a range ends in must equal, bit for bit, the state the next range
    //      started from -- so the concatenation is the sequential replay.  A range that fails the check
    //      (and everything after it) is replayed sequentially from the true state. ----
    const unsigned hw = std::thread::hardware_concurrency();
    int nthreads = (int)std::min<unsigned>(64, hw ? hw : 1);  // (16 until round 3: 13 ms for 28.8 M outputs)
    if (const char* ev = std::getenv("SIGOPS_REPLAY_THREADS")) nthreads = std::max(1, std::atoi(ev));  // tuning knob
    if (exact && nthreads > 1 && need - mcur >= ((int64_t)1 << 21) && L >= 2 && L <= 65536) {
        // a phase that is not a tie of the closed form (its position is >= 1/L away from an integer:
        // floor() there cannot depend on the drift) as range boundary
        int64_t r0 = -1;
        for (int64_t r = 1; r < L && r0 < 0; ++r)
            if ((r * ((int64_t)nphi * g.M)) % L != 0) r0 = r;
        const int64_t k0 = (mcur + L - 1) / L + 1;  // first whole period used as the reference
        if (r0 >= 0 && (k0 + 2) * L + r0 < need) {
            // sequentially up to the reference point and one period beyond it
            const int64_t mref = k0 * L + r0;
            run(mcur, mref, xb, acc, rec, memo0);
            const int64_t xb1 = xb;
            const double acc1 = acc;
            run(mref, mref + L, xb, acc, rec, memo0);
            const double dacc = acc - acc1;
            const int64_t dxb = xb - xb1;
            mcur = mref + L;
            const int64_t periods = (need - mcur) / L;
            const int nseg = (int)std::min<int64_t>(nthreads, periods / 1024);  // (ranges of >= 1024 periods: a thread's start costs ~30 us)
            if (nseg >= 2 && dxb == (int64_t)g.M * nphi) {
                struct Seg {
                    int64_t ma, mb, xb0, xb1;
                    double acc0, acc1;
                    Part part;
                };
                std::vector<Seg> seg(nseg);
                for (int t = 0; t < nseg; ++t) {
                    const int64_t ka = periods * t / nseg, kb = periods * (t + 1) / nseg;
                    seg[t].ma = mcur + ka * L;
                    seg[t].mb = t == nseg - 1 ? need : mcur + kb * L;
                    // predicted state before output ma (ma = mref + (1 + ka) L)
                    seg[t].xb0 = xb + ka * dxb;
                    seg[t].acc0 = acc + (double)ka * dacc;
                }
                t_r1 = std::chrono::steady_clock::now();
                std::vector<std::thread> th;
                int started = 0;
                try {
                    for (int t = 0; t < nseg; ++t) {
                        th.emplace_back([&, t] {
                            std::vector<int8_t> memo((size_t)nphi * 4, -1);
                            int64_t x = seg[t].xb0;
                            double a = seg[t].acc0;
                            seg[t].part.rec.reserve((size_t)((seg[t].mb - seg[t].ma) / L) * 2 + 64);
                            run(seg[t].ma, seg[t].mb, x, a, seg[t].part.rec, memo);
                            seg[t].xb1 = x;
                            seg[t].acc1 = a;
                            seg[t].part.ma = seg[t].ma;
                            seg[t].part.mb = seg[t].mb;
                            count_part(seg[t].part);
                        });
                        ++started;
                    }
                } catch (...) {  // (no more threads to be had: the ranges that did start still count)
                }
                for (auto& t : th) t.join();
                t_r2 = std::chrono::steady_clock::now();
                int good = 0;  // ranges whose start state has been confirmed
                for (int t = 0; t < started; ++t) {
                    const bool ok = t == 0 ? (seg[0].xb0 == xb && std::memcmp(&seg[0].acc0, &acc, 8) == 0)
                                           : (seg[t].xb0 == seg[t - 1].xb1 && std::memcmp(&seg[t].acc0, &seg[t - 1].acc1, 8) == 0);
                    if (!ok) break;
                    ++good;
                }
                if (good > 0) {  // (what ran in order so far is a piece of its own)
                    Part head;
                    head.rec.swap(rec);
                    head.ma = m0;
                    head.mb = mcur;
                    count_part(head);
                    parts.push_back(std::move(head));
                }
                for (int t = 0; t < good; ++t) {
                    parts.push_back(std::move(seg[t].part));
                    made.push_back(AccCheckpoint{seg[t].ma, seg[t].xb0, seg[t].acc0});
                    xb = seg[t].xb1;
                    acc = seg[t].acc1;
                    mcur = seg[t].mb;
                }
                if (std::getenv("SIGOPS_DEBUG_PLAN"))
                    std::fprintf(stderr, "[sigops] accumulator replay: %d of %d ranges confirmed (period drift %.3e)\n", good, nseg, dacc);
            }
        }
    }
    // the rest (everything, for short replays and rates without a period) in order
    while (mcur < need) {
        const int64_t mb = std::min<int64_t>(need, (mcur | (((int64_t)1 << 22) - 1)) + 1);
        if (mcur <= from && from < mb && from != mcur) {
            run(mcur, from, xb, acc, rec, memo0);
            mcur = from;
        }
        if (mcur == from) made.push_back(AccCheckpoint{mcur, xb, acc});
        run(mcur, mb, xb, acc, rec, memo0);
        mcur = mb;
        if (mcur < need) made.push_back(AccCheckpoint{mcur, xb, acc});
    }
    made.push_back(AccCheckpoint{need, xb, acc});
    t_r3 = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lock(g_acc_mu);
        std::vector<AccCheckpoint>* store = nullptr;
        for (auto& e : g_acc_checkpoints)
            if (e.first == ckey) store = &e.second;
        if (!store) {
            if (g_acc_checkpoints.size() >= 8) g_acc_checkpoints.erase(g_acc_checkpoints.begin());
            g_acc_checkpoints.emplace_back(ckey, std::vector<AccCheckpoint>{});
            store = &g_acc_checkpoints.back().second;
        }
        for (auto& c : made) {
            bool have = false;
            for (auto& o : *store) have = have || o.m == c.m;
            if (!have) store->push_back(c);
        }
        if (store->size() > 256) store->erase(store->begin(), store->begin() + (store->size() - 256));
    }
    {  // the rest in order: the last piece
        Part tail;
        tail.rec.swap(rec);
        tail.ma = parts.empty() ? m0 : parts.back().mb;
        tail.mb = need;
        count_part(tail);
        parts.push_back(std::move(tail));
    }
    size_t nrec = 0;
    for (const Part& pa : parts) nrec += pa.rec.size();
    if (bake && periodic) {
        // majority per period position among the deviations of the form (fine position - 1, α ≈ 1)
        std::vector<int64_t> cnt(L, 0);
        for (const Part& pa : parts)
            for (int64_t r = 0; r < L; ++r) cnt[r] += pa.cb[(size_t)r];
        prev.assign(L, 0);
        bool any = false;
        for (int64_t r = 0; r < L; ++r) {
            // (occurrences of period position r in [from, need); `from` is a multiple of L)
            const int64_t occ = need - from > r ? (need - from - 1 - r) / L + 1 : 0;
            if (occ > 0 && 2 * cnt[r] > occ) prev[r] = 1, any = true;
        }
        if (!any) prev.clear();
    }
    // fix-up list: deviations the tables do not already contain + outputs at baked positions
    // where the accumulator agreed with the closed form after all
    auto fdiv = [](int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };  // floor(a / b), b > 0
    if (!prev.empty()) {
        for (const Part& pa : parts) {
            const int64_t a = std::max(pa.ma, from), b = pa.mb;
            if (a >= b) continue;
            size_t in_tables = 0;  // records of this piece that are what the tables contain
            for (int64_t r = 0; r < L; ++r) {
                if (!prev[r]) continue;
                in_tables += (size_t)pa.cb[(size_t)r];
                // outputs of this piece at baked position r: every one with a record of its own?  (The usual case, decided by
                // the counts; otherwise the ones without are looked up.)
                const int64_t occ = fdiv(b - 1 - r, L) - fdiv(a - 1 - r, L);
                if (pa.ca[(size_t)r] == occ) continue;
                size_t k = 0;
                int64_t m = a + ((r - a % L) % L + L) % L;
                for (; m < b; m += L) {
                    while (k < pa.rec.size() && pa.rec[k].m < m) ++k;
                    if (k < pa.rec.size() && pa.rec[k].m == m) continue;  // deviates: baked, or listed below
                    const int64_t q = exact_q(m), Nn = m * ((int64_t)nphi * g.M);
                    fix.push_back(RsFix{m, q / nphi, (int32_t)(q % nphi), 0, (double)(Nn % L) / (double)L});
                }
            }
            if (in_tables == pa.rec.size()) continue;
            for (const Rec& r : pa.rec) {
                if (prev[r.m % L] && baked(r)) continue;  // what the tables contain
                fix.push_back(RsFix{r.m, r.qa / nphi, (int32_t)(r.qa % nphi), 0, r.alpha});
            }
        }
    } else {
        for (const Part& pa : parts)
            for (const Rec& r : pa.rec) fix.push_back(RsFix{r.m, r.qa / nphi, (int32_t)(r.qa % nphi), 0, r.alpha});
    }
    std::sort(fix.begin(), fix.end(), [](const RsFix& a, const RsFix& b) { return a.m < b.m; });
    if (from > 0) {
        const int64_t jin = exact ? from / L * g.M : g.j0;  // (what the stage's first staged input frame is)
        for (auto& f : fix) {
            f.m -= from;
            f.j -= jin;
        }
    }
    if (std::getenv("SIGOPS_DEBUG_PLAN")) {
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "[sigops] accumulator replay of %lld outputs: head %.3f ms, ranges in threads %.3f, rest in order %.3f, lists %.3f (%zu deviations, %zu fix-ups)\n",
                     (long long)(need - from), ms(t_r0, t_r1), ms(t_r1, t_r2), ms(t_r2, t_r3), ms(t_r3, std::chrono::steady_clock::now()), nrec, fix.size());
    }
}

// integer frame rates: the arbitrary-rate kernel's rate is the exact rational fs_out/fs_in
void rs_detect_exact(RsGeom& g, double fo, double fi, double rate) {
    if (fo == std::floor(fo) && fi == std::floor(fi) && fo >= 1 && fi >= 1 && fo < 2147483648.0 &&
        fi < 2147483648.0 && fo / fi == rate) {
        int64_t a = (int64_t)fo, b = (int64_t)fi;
        while (b) {
            int64_t t = a % b;
            a = b;
            b = t;
        }
        int64_t Lx = (int64_t)fo / a, Mx = (int64_t)fi / a;
        if (Lx <= 8192 && Mx <= 1048576) {
            g.exact = 1;
            g.L = Lx;
            g.M = Mx;
        }
    }
}

// Diagnostics (host only): the (newest input, phase, alpha) the arbitrary-rate resampler kernels
// use for outputs [0,n_out) -- closed form, baked period positions and fix-up list combined.
int resample_positions(double fs_in, double fs_out, double rate, int nphi, const double* h, int hlen,
                       int64_t n_out, int64_t* jo, int32_t* po, double* ao, int64_t* nfix, int64_t* nbaked) {
    RsGeom g{};
    g.arbitrary = 1;
    g.nphi = nphi;
    g.delta = (double)nphi / rate;
    g.c0 = (double)(hlen - 1) / 2.0;
    g.c0i = (hlen - 1) / 2;
    g.taps = (hlen + nphi - 1) / nphi;
    rs_detect_exact(g, fs_out, fs_in, rate);
    std::vector<uint8_t> prev;
    std::vector<RsFix> fix;
    const auto t0 = std::chrono::steady_clock::now();
    if (!std::getenv("SIGOPS_RS_EXACT")) replay_phase_accumulator(g, h, hlen, n_out, g.exact && n_out >= 2048, prev, fix);
    if (std::getenv("SIGOPS_DEBUG_PLAN"))
        std::fprintf(stderr, "[sigops] phase accumulator replay: %lld outputs, %.1f ms\n", (long long)n_out,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    for (int64_t m = 0; m < n_out; ++m) {
        int64_t qi;
        double alpha;
        if (g.exact) {
            const int64_t Nn = m * ((int64_t)nphi * g.M);
            qi = g.c0i + Nn / g.L;
            alpha = (double)(Nn % g.L) / (double)g.L;
            if (!prev.empty() && prev[m % g.L]) {
                qi -= 1;
                alpha = 1.0;
            }
        } else {
            const double t = (double)m * g.delta;
            const double q = g.c0 + t;
            const double fl = std::floor(q);
            qi = (int64_t)fl;
            alpha = q - fl;
        }
        jo[m] = qi / nphi;
        po[m] = (int32_t)(qi % nphi);
        ao[m] = alpha;
    }
    for (const RsFix& f : fix) {
        jo[f.m] = f.j;
        po[f.m] = f.p;
        ao[f.m] = f.alpha;
    }
    if (nfix) *nfix = (int64_t)fix.size();
    if (nbaked) {
        *nbaked = 0;
        for (uint8_t b : prev) *nbaked += b;
    }
    return SO_OK;
}


}  // namespace so
