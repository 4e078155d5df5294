// pass2_mc.hip -- pass 2 with the transforms on the matrix cores (mcdft.h):
// rDFT recompute + w^H x + inverse rDFT + window + overlap-add.
//
// Replaces (funcwj/setk): Beamformer.beamform (libs/beamformer.py:220-234),
// post-masking (apply_adaptive_beamformer.py:174-175) and inverse_stft
// (libs/utils.py:142-173 -> librosa.istft 0.8.1: irfft, * window, overlap-add,
// / sum(window^2) where > tiny, trim n_fft/2; the inf-norm rescale is scale_kernel).
//
// One wavefront owns a run of consecutive frames, two frames (a group) at a time: it transforms
// the C channels one after the other, both frames of a channel as a pair (24 MFMA; every operand
// tile, window row and twiddle row read from LDS once for the two; the next channel's twelve
// samples per lane in flight), folds conj(w_c) X_c into four complex accumulators per lane and
// frame (the lane's bins are fixed, its weights come from an LDS table as one base address +
// immediates), adds the odd family X[16 + 32 q] of all channels of both frames from ONE extra
// tile per group, scales each frame's spectrum by a power of two into the fp16 operand range,
// inverse-transforms the pair (24 MFMA over one read of the inverse's tiles), windows, and
// completes one block of hop output samples per frame from its own registers (hop = n_fft / 2:
// see the kernel).  No frame slots, no
// workgroup barrier, no overlap-add loop; ~128 VGPRs: four waves per SIMD where the butterfly
// kernel ran two.  Other hops keep pass2.hip.
#include "common.h"
#include "fft512.h"
#include "mcdft.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace setk {

// float32 form: two 512-thread workgroups per CU.  16-bit PCM form: ONE 1024-thread workgroup
// per CU (the tables once instead of twice) whose waves carry the group-boundary half frame of
// every channel through LDS as packed int16 (8 bytes per lane and channel = 4 KB per wave)
// instead of re-reading it from HBM at the next group -- the re-read was 1/3 of the kernel's
// audio traffic (counter traffic 1.35 x algorithmic).  The same carry for float32 samples (16
// bytes per lane and channel, four channels at most) measured 6.6 % SLOWER in stage 3 at MORE
// traffic (profiles/rejected/round6_pass2_f32_partial_carry_ab.txt).
constexpr int kP2McWavesPerSimd = 4;
constexpr int kP2McGroup = 2;  // R: consecutive frames per group (the carry is written for two)
constexpr int p2mc_threads(bool pcm) { return pcm ? 1024 : 512; }

// forward operand tiles, window rows and twiddles in LDS: BR_H .. IT_L (10 tiles, contiguous
// words) + OT_H, OT_L + the forward's 8 + window 2 + twiddles 3
constexpr int kP2McTiles = 25;
// LDS plan (bytes): wtab C * 257 * 8 | operand tiles 25 * 1024 | synthesis rows
// 2048 | a16 scratch NW * R * 8 * kOddPitch * 4 | yodd NW * R * 16 * 4 | red 64
// | PCM carry NW * C * 64 * 8
size_t pass2_mc_lds_bytes(int C, bool pcm) {
    const size_t nw = p2mc_threads(pcm) / 64;
    const size_t wt = ((size_t)C * kBins * sizeof(cf) + 15) & ~(size_t)15;
    return wt + kP2McTiles * 1024 + 2048 + nw * kP2McGroup * 8 * mc::kOddPitch * sizeof(float) +
           nw * kP2McGroup * 16 * sizeof(float) + 64 + (pcm ? nw * C * 64 * sizeof(uint2) : 0);
}

// sum over each 8-lane half of every 16-lane row on its own (the three steps stay inside a half),
// result in all lanes of the half: lanes 0..7 = frame 0 of a group, 8..15 = frame 1
SETK_DEV float row8_sum(float x) {
    int v = __builtin_bit_cast(int, x);
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true));   // j ^ 1
    v = __builtin_bit_cast(int, x);
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true));   // j ^ 2
    v = __builtin_bit_cast(int, x);
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true));  // j ^ 7
    return x;
}
// max over the 64 lanes (values >= 0), wave-uniform result
SETK_DEV float wave_max_nonneg(float x) {
    int v = __builtin_bit_cast(int, x);
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true)));
    v = __builtin_bit_cast(int, x);
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true)));
    v = __builtin_bit_cast(int, x);
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true)));
    v = __builtin_bit_cast(int, x);
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true)));
    const unsigned b = __builtin_bit_cast(unsigned, x);
    unsigned m = __builtin_amdgcn_readlane(b, 0);
    const unsigned m1 = __builtin_amdgcn_readlane(b, 16), m2 = __builtin_amdgcn_readlane(b, 32),
                   m3 = __builtin_amdgcn_readlane(b, 48);
    m = m > m1 ? m : m1;  // non-negative floats order like their bit patterns
    m = m > m2 ? m : m2;
    m = m > m3 ? m : m3;
    return __builtin_bit_cast(float, m);
}

// hop = n_fft / 2 (the CLI's default geometry): every output block of `hop` samples is the sum
// of exactly two frame halves, so a wavefront that walks CONSECUTIVE frames carries the second
// half of its last frame in four registers per lane and finishes a block per frame by itself --
// no frame slots in LDS, no workgroup barrier, no overlap-add loop.  1 / sum(window^2) is folded
// into the synthesis rows (mc_syn); blocks with a single contribution (the first and the last
// one of an utterance, emitted only when center = False) take the per-lane corrections mc_edge.
// A workgroup shares the weight table and the once-per-frame operand tiles; its waves split the
// item's frame range and each recomputes one frame ahead of its sub-range for the carry.
// PCM: UttDesc::audio is planar 16-bit PCM (kAudioPcm16) -- sign-extending 2-byte loads, one
// conversion per sample, and 2^-15 (read_wav's int16 / 32768) folded into the window rows.
template <int C, bool PCM = false>
__global__ __launch_bounds__(p2mc_threads(PCM), kP2McWavesPerSimd) void beamform_istft_mc_kernel(Pass2Args a) {
    constexpr int NT = p2mc_threads(PCM);
    constexpr int NW = NT / 64;
    constexpr int F = kBins;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* p = smem;
    cf* wtab = reinterpret_cast<cf*>(p);  // [C][257]
    p += ((size_t)C * F * sizeof(cf) + 15) & ~(size_t)15;
    // [25][64]: BR_H BR_L BI_H BI_L G0_H G0_L G1_H G1_L IT_H IT_L OT_H OT_L | the forward's 8 |
    // window rows 0..3, 4..7 | TR TI TRI
    mc::u4* tiles = reinterpret_cast<mc::u4*>(p);
    p += kP2McTiles * 1024;
    mc::f4* synr = reinterpret_cast<mc::f4*>(p);  // [2][64] float4: synthesis rows 0..3 / 4..7 of a lane
    p += 2048;
    float* a16s = reinterpret_cast<float*>(p);  // [NW][R][8][kOddPitch]
    p += (size_t)NW * kP2McGroup * 8 * mc::kOddPitch * sizeof(float);
    float* yodd_s = reinterpret_cast<float*>(p);  // [NW][R][16]
    p += NW * kP2McGroup * 16 * sizeof(float);
    float* red = reinterpret_cast<float*>(p);
    p += 64;
    uint2* carry_s = reinterpret_cast<uint2*>(p);  // PCM: [NW][C][64] packed int16 x 4

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const WorkItem wi = a.items[blockIdx.x];
    const UttDesc ud = a.utts[wi.utt];
    const int n_samp = ud.num_samples;
    const int T = ud.num_frames;
    const int hop = kNfft / 2;
    const bool post_mask = (a.flags & 0x4) != 0;
    const bool clamp = (a.flags & 0x2) != 0;

    // The fp16 operand splits of the forward transform hold window x sample x 2^10 and want
    // |sample| <= 1 (65504 is the end of fp16).  The utterance's max |x| is known (pass 1 reduced
    // it into norm_bits before this kernel started): samples above 1 -- float wave files, int16
    // ranges handed over as floats (WaveReader(normalize=False)), C-API callers -- are brought
    // into range by the power of two 2^-e in the window rows and taken out again by 2^e in the
    // synthesis rows.  The other way round for an utterance that is quiet throughout: below
    // 2^-10 of full scale the lo halves of the splits go subnormal (an absolute floor of 2^-34
    // per sample, mcdft.h), so max |x| < 2^-15 -- less than one step of 16-bit PCM, float input
    // only -- is lifted by the same exact power of two (tests/stft_cases.py `quiet`: without it
    // the wave of an utterance peaking at 2^-24 came out 6e-4 off, at 2^-32 0.15, against the
    // 1e-3 waveform bar; with it 2e-7).  e = 0 (nothing changes, bit for bit)
    // whenever 2^-15 <= max |x| <= 1, and for silence.  The beamformer is linear, every other
    // stage of this kernel is scale free (the inverse transform normalises each frame's
    // spectrum by its own power of two).  16-bit PCM arrives as integers: 2^-15 on the way in,
    // nothing on the way out.
    float in_sc = PCM ? 3.0517578125e-05f : 1.f, out_sc = 1.f;
    if (a.norm_bits) {
        const unsigned nb = a.norm_bits[wi.utt];  // max |x| (natural units) as float bits
        const float mx = __builtin_bit_cast(float, nb);
        int e = (int)((nb >> 23) & 0xff) - 126;   // max |x| < 2^e
        e = (mx > 1.f) ? (e > 100 ? 100 : e) : (mx > 0.f && mx < 3.0517578125e-05f) ? (e < -100 ? -100 : e) : 0;
        in_sc *= __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
        out_sc = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
    }
    {
        const cf* wsrc = reinterpret_cast<const cf*>(a.weight) + (size_t)wi.utt * C * kBinsPad;
        for (int i = tid; i < C * F; i += NT) {
            const int c = i / F, f = i - c * F;
            wtab[i] = wsrc[c * kBinsPad + f];
        }
    }
    mc::stage_tiles(tiles, a.mc_tab, mc::kW_BR_H, 10, tid, NT);
    mc::stage_tiles(tiles + 10 * 64, a.mc_tab, mc::kW_OT_H, 2, tid, NT);
    mc::stage_tiles(tiles + 12 * 64, a.mc_tab, mc::kW_MC_H, 8, tid, NT);
    for (int i = tid; i < 128; i += NT) {
        const int l = i & 63, t4 = i >> 6;
        const mc::f4 w = {a.mc_win[(4 * t4 + 0) * 64 + l] * in_sc, a.mc_win[(4 * t4 + 1) * 64 + l] * in_sc,
                          a.mc_win[(4 * t4 + 2) * 64 + l] * in_sc, a.mc_win[(4 * t4 + 3) * 64 + l] * in_sc};
        tiles[20 * 64 + i] = __builtin_bit_cast(mc::u4, w);
    }
    mc::stage_tiles(tiles + 22 * 64, a.mc_tab, mc::kW_TR, 3, tid, NT);
    for (int i = tid; i < 128; i += NT) {
        const int l = i & 63, hf = i >> 6;
        synr[i] = (mc::f4){a.mc_syn[(4 * hf + 0) * 64 + l] * out_sc, a.mc_syn[(4 * hf + 1) * 64 + l] * out_sc,
                           a.mc_syn[(4 * hf + 2) * 64 + l] * out_sc, a.mc_syn[(4 * hf + 3) * 64 + l] * out_sc};
    }
    struct { float tr[4], ti[4]; } K;  // (the inverse's conjugate twiddles: re-read there)
    float* yoddw = yodd_s + wave * kP2McGroup * 16;  // [R][16]
    const int lane_bin = mc::bin_of(c16, g, 0);
    const cf* wl = wtab + lane_bin;                       // + c * F + 32 r
    const int lane_n = 64 * g + c16;                      // sample 16 (4 g + r) + n2 = lane_n + 16 r
    float omax = 0.f;
    __syncthreads();  // tables ready (the only workgroup barrier before the epilogue)

    // this wave's frames [ta, tb); one frame ahead of ta is recomputed for its second half
    const int per = (wi.t1 - wi.t0 + NW - 1) / NW;
    const int ta = wi.t0 + wave * per;
    const int tb = min(ta + per, wi.t1);
    const int tw = ta > 0 ? ta - 1 : ta;  // first frame computed

    // Channel-major over groups of R consecutive frames: with hop = n_fft / 2 frame t + 1 shares
    // its first half with frame t -- the same lane's registers (mc::sample_of) -- so inside a
    // group's pair of transforms takes twelve samples per lane, not sixteen, and the weights, the
    // operand tiles and the table rows of a channel are read once per group.  The R spectra of the
    // group accumulate in registers.
    constexpr int R = kP2McGroup;
    float* a16g = a16s + wave * R * 8 * mc::kOddPitch;  // [R][8 channels][kOddPitch]
    float carry[4] = {0.f, 0.f, 0.f, 0.f};
    // EDGE (load_pair): some sample of the group lies outside the signal (numpy "reflect" padding) -- the
    // first and the last group of an utterance; frames past the last one repeat it (computed
    // to keep the group uniform, never emitted).
    // channel c of the utterance: float32 [C][N] or int16 [C][ch_stride] (the conversion is the
    // implicit one of `float = short`: global_load_sshort + v_cvt_f32_i32)
    auto chan = [&](int c) {
        if constexpr (PCM) return (gcshort_p)gptr(ud.audio) + (size_t)c * ud.ch_stride;
        else return gptr(ud.audio) + (size_t)c * n_samp;
    };
    // PCM carry: the lane's own four samples of the half frame a group ends with, per channel --
    // a thread reads back exactly what it wrote (program order suffices, no barrier)
    uint2* carry_l = carry_s + (size_t)wave * C * 64 + lane;  // + 64 c
    // loader: the two frames of a group of channel c -- three half frames, 12 samples per lane
    // (v[0..3], v[4..7]: frame t0; v[4..7], v[8..11]: frame t0 + 1).  PCM: the last half frame
    // stays raw in nr (it is packed for the carry where it is consumed), v[8..11] are unused.
    auto load_pair = [&](float (&v)[12], int (&nr)[4], int t0, int c, auto edge) __attribute__((always_inline)) {
        const auto x = chan(c);
        const int o = 64 * g + c16;
        const int s0 = min(t0, T - 1) * hop - a.g.pad, s1 = min(t0 + 1, T - 1) * hop - a.g.pad + 256;
        // interior addresses, from three channels up: a wave-uniform base per half frame, opaque so
        // that it stays in scalar registers, and the lane's unsigned offset.  Left to itself the
        // compiler folds the lane's part into a 64-bit address per lane, a loop invariant that
        // the request sites of the channel loop push into scratch; with one or two channels it
        // does better left to itself (profiles/no_copies/resource_usage.txt).
        auto base = [&](int s) __attribute__((always_inline)) {
            auto xs = x + s;
            if constexpr (C > 2) asm volatile("" : "+s"(xs));
            return xs;
        };
        const auto xa = base(s0), xb = base(s1);
        auto at = [&](decltype(xa) xs, int s, int k) __attribute__((always_inline)) {
            if constexpr (C > 2) return xs + ((unsigned)o + (unsigned)k);
            else return x + (s + o + k);
        };
        if constexpr (PCM) {
            // first half: what this lane parked at the end of the previous group (or the prefill
            // before the first); the other two: the only samples of the group not seen yet
            const uint2 pk = carry_l[64 * c];
            v[0] = (float)(short)(pk.x & 0xffff);
            v[1] = (float)((int)pk.x >> 16);
            v[2] = (float)(short)(pk.y & 0xffff);
            v[3] = (float)((int)pk.y >> 16);
            if (!decltype(edge)::value) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[4 + e] = *at(xa, s0, 256 + 16 * e);
                    nr[e] = *at(xb, s1, 16 * e);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[4 + e] = x[reflect_index(s0 + o + 256 + 16 * e, n_samp)];
                    nr[e] = x[reflect_index(s1 + o + 16 * e, n_samp)];
                }
            }
        } else {
            if (!decltype(edge)::value) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // both halves of a group's first frame are read for the last time here (the
                    // first one is the re-read of what the previous group fetched as ITS last
                    // half): a streaming hint keeps them from pushing the halves that WILL be read
                    // again -- the group's last -- out of the XCD's L2
                    v[e] = __builtin_nontemporal_load(at(xa, s0, 16 * e));
                    v[4 + e] = __builtin_nontemporal_load(at(xa, s0, 256 + 16 * e));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[8 + e] = *at(xb, s1, 16 * e);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = x[reflect_index(s0 + o + 16 * e, n_samp)];
                    v[4 + e] = x[reflect_index(s0 + o + 256 + 16 * e, n_samp)];
                    v[8 + e] = x[reflect_index(s1 + o + 16 * e, n_samp)];
                }
            }
        }
    };
    mc::f4 yr[R], yi[R];
    // the pair of transforms of every channel of one group.  Two sample buffers swap roles from
    // channel to channel: a channel's pair is transformed out of `cur` in place while the next
    // channel's samples travel into `nx` (one buffer cost twelve v_mov_b32 per channel to move
    // the arrivals out of the way of the next request, profiles/no_copies/census.txt).  Buffer a
    // arrives holding the group (t0, channel 0) and leaves holding (t0 + R, channel 0) once
    // request_group has run.
    static_assert(R == 2, "the paired transform and the LDS carry are written for groups of two frames");
    // The second buffer is worth its twelve registers where the loop then still fits the 128:
    // float32 input from five channels up.  With two to four channels and for PCM input (nraw
    // doubles too) it pushed one to three registers of the prologue into scratch, so those keep
    // the one buffer (profiles/no_copies/resource_usage.txt).
    constexpr bool kTwoBuf = !PCM && C >= 5;
    float buf_a[12], buf_b[12];
    int nraw_a[4], nraw_b[4];  // PCM: the group's last half frame, as loaded
    // one channel; `more`: channel c + 1 exists and is requested
    auto channel = [&](const float (&cur)[12], const int (&craw)[4], float (&nx)[12], int (&nxraw)[4], int t0,
                       int c, bool more, auto edge) __attribute__((always_inline)) {
        float x0[8], x1[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x0[e] = cur[e];
            x0[4 + e] = cur[4 + e];
            x1[e] = cur[4 + e];
            if constexpr (PCM) x1[4 + e] = (float)craw[e];
            else x1[4 + e] = cur[8 + e];
        }
        if constexpr (PCM) {
            // the group's last half frame is the next group's first
            carry_l[64 * c] = make_uint2(__builtin_amdgcn_perm((unsigned)craw[1], (unsigned)craw[0], 0x05040100u),
                                         __builtin_amdgcn_perm((unsigned)craw[3], (unsigned)craw[2], 0x05040100u));
        }
        // the next channel's twelve samples travel while this pair runs (the next group's
        // channel 0 is requested after the group: its span decides the path)
        if (more) load_pair(nx, nxraw, t0, c + 1, edge);
        mc::f4 zr0, zi0, a16_0, zr1, zi1, a16_1;
        {
            asm volatile("" ::: "memory");  // tiles and tables: once per channel and group, not kept
            const mc::f4 w0 = __builtin_bit_cast(mc::f4, tiles[20 * 64 + lane]);
            const mc::f4 w1 = __builtin_bit_cast(mc::f4, tiles[21 * 64 + lane]);
            const float win[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
            mc::forward2_t(x0, x1, win, [&](int i) { return mc::lds_h8(tiles, 12 + i, lane); },
                           [&](int i) { return __builtin_bit_cast(mc::f4, tiles[(22 + i) * 64 + lane]); },
                           zr0, zi0, a16_0, zr1, zi1, a16_1);
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");  // the weights are re-read per group, not kept (64 registers)
        const cf* wc = wl + c * F;
        cf w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = wc[32 * r];
        mc::store_a16(a16g, c, lane, a16_0);
        mc::store_a16(a16g + 8 * mc::kOddPitch, c, lane, a16_1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yr[0][r] = fmaf(zr0[r], w[r].x, fmaf(zi0[r], w[r].y, yr[0][r]));
            yi[0][r] = fmaf(zi0[r], w[r].x, fmaf(-zr0[r], w[r].y, yi[0][r]));
            yr[1][r] = fmaf(zr1[r], w[r].x, fmaf(zi1[r], w[r].y, yr[1][r]));
            yi[1][r] = fmaf(zi1[r], w[r].x, fmaf(-zr1[r], w[r].y, yi[1][r]));
        }
        // the fold stays with its channel (an empty statement that claims the sums: with two
        // channels in one loop body the compiler otherwise sinks this fold below the next
        // channel's transforms and keeps sixteen spectrum registers alive across them)
        if constexpr (kTwoBuf) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                asm volatile("" : "+v"(yr[k][0]), "+v"(yr[k][1]), "+v"(yr[k][2]), "+v"(yr[k][3]),
                                  "+v"(yi[k][0]), "+v"(yi[k][1]), "+v"(yi[k][2]), "+v"(yi[k][3]));
            }
        }
        // one pair at a time: the scheduler must not pull the next channel's pair in
        __builtin_amdgcn_sched_barrier(0);
    };
    auto group = [&](int t0, auto edge) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            yr[k] = (mc::f4){0.f, 0.f, 0.f, 0.f};
            yi[k] = (mc::f4){0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (decltype(edge)::value || !kTwoBuf) {
            // one buffer, refilled in place: the first and the last group of an utterance (the
            // reflect indexing of three request sites would cost more registers than the moves),
            // and every group of the instantiations outside kTwoBuf
#pragma unroll 1
            for (int c = 0; c < C; ++c) channel(buf_a, nraw_a, buf_a, nraw_a, t0, c, c + 1 < C, edge);
        } else {
            // channels two at a time, a -> b -> a; the last one or two stand outside the loop,
            // so that inside it every channel requests its successor unconditionally
            int c = 0;
#pragma unroll 1
            for (; c + 2 < C; c += 2) {
                channel(buf_a, nraw_a, buf_b, nraw_b, t0, c, true, edge);
                channel(buf_b, nraw_b, buf_a, nraw_a, t0, c + 1, true, edge);
            }
            if constexpr (C % 2 == 0) {
                channel(buf_a, nraw_a, buf_b, nraw_b, t0, c, true, edge);
                channel(buf_b, nraw_b, buf_a, nraw_a, t0, c + 1, false, edge);
            } else {
                channel(buf_a, nraw_a, buf_b, nraw_b, t0, c, false, edge);
            }
        }
    };
    auto span_is_edge = [&](int t0) {
        const int lo = t0 * hop - a.g.pad, hi = (t0 + R - 1) * hop - a.g.pad + kNfft;
        return lo < 0 || hi > n_samp || t0 + R > T;
    };
    auto request_group = [&](int t0) __attribute__((always_inline)) {
        if (span_is_edge(t0)) load_pair(buf_a, nraw_a, t0, 0, std::true_type());
        else load_pair(buf_a, nraw_a, t0, 0, std::false_type());
    };
    if constexpr (PCM) {
        // the first half of the wave's first frame, every channel: from here on a group reads two
        // half frames per channel from HBM, never three
        if (tw < tb) {
#pragma unroll 1
            for (int c = 0; c < C; ++c) {
                const auto x = chan(c);
                const int s0 = tw * hop - a.g.pad, o = 64 * g + c16;
                int r[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = x[reflect_index(s0 + o + 16 * e, n_samp)];
                carry_l[64 * c] = make_uint2(__builtin_amdgcn_perm((unsigned)r[1], (unsigned)r[0], 0x05040100u),
                                             __builtin_amdgcn_perm((unsigned)r[3], (unsigned)r[2], 0x05040100u));
            }
        }
    }
    if (tw < tb) request_group(tw);
#pragma unroll 1
    for (int t0 = tw; t0 < tb; t0 += R) {
        const int nf = min(R, tb - t0);
        // (the channels 1.. of this group are fetched inside it: from the carry unless it is the
        //  wave's first group)
        if (span_is_edge(t0)) group(t0, std::true_type());
        else group(t0, std::false_type());
        if (t0 + R < tb) request_group(t0 + R);  // (issued here: its span decides the path)
        // ---- the tail of both frames at once: every once-per-frame tile is read once per group.
        //      Frame 1 of a short group (nf < R) is computed and dropped. ----
        const int t1 = min(t0 + 1, T - 1);  // (the mask row of a frame past the end: any valid one)
        // the lane's once-per-group addresses are formed here from an opaque copy of the lane
        // index (a dozen integer operations per group): as loop invariants they take registers
        // the transforms need and end up in scratch
        int lt = lane;
        asm volatile("" : "+v"(lt));
        const int kf = (lt >> 3) & 1, co = lt & 7, c16 = lt & 15, g = lt >> 4;  // odd-family tile: column = 8 x frame + channel
        const bool odd_on = co < C;
        const cf* wo = wtab + (odd_on ? co : 0) * F + 16 + 64 * g;  // w_j[16 + 32 (2 g)], [+ 32] the next
        const int orow = 8 * kf + (odd_on ? co : C - 1);            // unused columns repeat a valid row
        // ---- odd family of all channels of both frames: ONE tile, column 8 k + c = frame k,
        //      channel c; then the sum over the channel lanes of each 8-lane half ----
        float yo[4];
        {
            asm volatile("" ::: "memory");  // the once-per-group tiles are re-read, not kept
            const mc::f4 d = mc::odd_tile_row(a16g, mc::lds_h8(tiles, 10, lane), mc::lds_h8(tiles, 11, lane), lane, orow);
            const cf w0 = wo[0], w1 = wo[32];
            yo[0] = odd_on ? fmaf(d[0], w0.x, d[1] * w0.y) : 0.f;
            yo[1] = odd_on ? fmaf(d[1], w0.x, -d[0] * w0.y) : 0.f;
            yo[2] = odd_on ? fmaf(d[2], w1.x, d[3] * w1.y) : 0.f;
            yo[3] = odd_on ? fmaf(d[3], w1.x, -d[2] * w1.y) : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) yo[i] = row8_sum(yo[i]);
        }
        mc::f4 fr[R], fi[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            fr[k] = yr[k];
            fi[k] = yi[k];
        }
        // ---- optional post-mask ----
        if (post_mask) {
            const float* mrow = ud.mask_s + (size_t)t0 * F;
            // the lane's offsets are formed here, against the row's scalar base: hoisted out of
            // the group loop they are 64-bit addresses per lane that live in scratch
            const unsigned dm = (unsigned)(t1 - t0) * F;  // frame 1's row
            unsigned mo = (unsigned)lane_bin, mq = 16u + 64u * (unsigned)g + (kf ? dm : 0u);
            asm volatile("" : "+v"(mo), "+v"(mq));
#pragma unroll
            for (int k = 0; k < R; ++k) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float m = mrow[mo + (k ? dm : 0u) + 32 * r];
                    if (clamp) m = fminf(m, 1.f);
                    fr[k][r] *= m;
                    fi[k][r] *= m;
                }
            }
            float m0 = mrow[mq], m1 = mrow[mq + 32];
            if (clamp) { m0 = fminf(m0, 1.f); m1 = fminf(m1, 1.f); }
            yo[0] *= m0;
            yo[1] *= m0;
            yo[2] *= m1;
            yo[3] *= m1;
        }
        // ---- power-of-two scale of each frame into the fp16 operand range: max < 2^11 ----
        const float yom = fmaxf(fmaxf(fabsf(yo[0]), fabsf(yo[1])), fmaxf(fabsf(yo[2]), fabsf(yo[3])));
        float sc[R], isc[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            // only Re Y[0], Re Y[256] reach the inverse (numpy irfft drops their imaginary parts)
            fi[k][0] = (lane == 0) ? 0.f : fi[k][0];
            fi[k][3] = (lane == 32) ? 0.f : fi[k][3];
            float mxl = (kf == k) ? yom : 0.f;  // the odd family of frame k sits in its half of the rows
#pragma unroll
            for (int r = 0; r < 4; ++r) mxl = fmaxf(mxl, fmaxf(fabsf(fr[k][r]), fabsf(fi[k][r])));
            const float mxw = wave_max_nonneg(mxl);
            int ex = (int)((__builtin_bit_cast(unsigned, mxw) >> 23) & 0xff);  // mxw < 2^(ex - 126)
            ex = ex < 16 ? 16 : (ex > 250 ? 250 : ex);                         // (zero / tiny / huge frames)
            sc[k] = __builtin_bit_cast(float, (unsigned)(264 - ex) << 23);     // 2^(137 - ex)
            isc[k] = __builtin_bit_cast(float, (unsigned)(ex - 10) << 23);
        }
        // ---- E16 of the odd family: its tile takes frames as rows; the group's are rows 0, 1 ----
        {
            const float scl = kf ? sc[1] : sc[0];
            if ((c16 & 7) == 0) *reinterpret_cast<mc::f4*>(yoddw + 16 * kf + 4 * g) = (mc::f4){yo[0] * scl, yo[1] * scl, yo[2] * scl, yo[3] * scl};
        }
        float e16[R];
        {
            float v[8];
            const mc::f4 v0 = *reinterpret_cast<const mc::f4*>(yoddw + 16 * (c16 & 1) + 8 * (g & 1));
            const mc::f4 v1 = *reinterpret_cast<const mc::f4*>(yoddw + 16 * (c16 & 1) + 8 * (g & 1) + 4);
            const float rowsel = c16 < R ? 1.f : 0.f;  // rows 2..15 of the tile are unused
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = v0[e] * rowsel;
                v[4 + e] = v1[e] * rowsel;
            }
            const mc::f4 d = mc::inv_odd_tile(v, mc::lds_h8(tiles, 8, lane), mc::lds_h8(tiles, 9, lane), lane);
            e16[0] = d[0];  // lanes g == 0: E16[n2 = l % 16] of row 0, row 1
            e16[1] = d[1];
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                fr[k][r] *= sc[k];
                fi[k][r] *= sc[k];
            }
        }
        float bmid0[8], bmid1[8];
        {
            const mc::f4 tt0 = __builtin_bit_cast(mc::f4, tiles[22 * 64 + lane]);
            const mc::f4 tt1 = __builtin_bit_cast(mc::f4, tiles[23 * 64 + lane]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                K.tr[r] = tt0[r];
                K.ti[r] = tt1[r];
            }
        }
        auto inv_tile = [&](int i) { return mc::lds_h8(tiles, i, lane); };
        mc::inverse2_a(fr[0], fi[0], e16[0], fr[1], fi[1], e16[1], inv_tile, K.tr, K.ti, bmid0, bmid1, lane);
        asm volatile("" ::: "memory");
        mc::f4 y0[R], y1[R];
        mc::inverse2_b(bmid0, bmid1, inv_tile, y0[0], y1[0], y0[1], y1[1]);
        // ---- block t = first half of frame t + second half of frame t - 1 (the carry); the
        //      rows hold window / 512 / sum(window^2) x the back-scale of the spectra ----
        const mc::f4 s0 = synr[lane], s1 = synr[64 + lane];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (k >= nf) break;
            const int t = t0 + k;
            float blk[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) blk[r] = fmaf(y0[k][r], s0[r] * isc[k], carry[r]);
            if (t == 0) {  // no frame before the first: a single contribution (center = False only)
#pragma unroll
                for (int r = 0; r < 4; ++r) blk[r] *= gptr(a.mc_edge)[r * 64 + lane];
            }
            if (t >= ta) {
                const int o = t * hop - a.g.pad + lane_n;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int oo = o + 16 * r;
                    if (oo >= 0 && oo < ud.out_len) {
                        ud.wave_f32[oo] = blk[r];
                        omax = fmaxf(omax, fabsf(blk[r]));
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) carry[r] = y1[k][r] * (s1[r] * isc[k]);
        }
    }
    // ---- the block after the last frame: its second half alone (center = False only) ----
    if (tb == T && ta < tb) {
        const int o = T * hop - a.g.pad + lane_n;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int oo = o + 16 * r;
            const float v = carry[r] * gptr(a.mc_edge)[(4 + r) * 64 + lane];
            if (oo >= 0 && oo < ud.out_len) {
                ud.wave_f32[oo] = v;
                omax = fmaxf(omax, fabsf(v));
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) omax = fmaxf(omax, __shfl_xor(omax, o));
    if ((tid & 63) == 0) red[tid >> 6] = omax;
    __syncthreads();
    if (tid == 0) {
        float m = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, red[w]);
        atomicMax(a.outmax_bits + wi.utt, __float_as_uint(m));
    }
}

// workgroups of this kernel a CU holds (registers and LDS), for the work-list cut of capi.hip
int pass2_mc_wgs_per_cu(int C, bool pcm) {
    const int by_waves = kP2McWavesPerSimd * 4 / (p2mc_threads(pcm) / 64);
    const int by_lds = (int)((160u << 10) / pass2_mc_lds_bytes(C, pcm));
    return by_waves < by_lds ? (by_waves > 0 ? by_waves : 1) : (by_lds > 0 ? by_lds : 1);
}

template <int C, bool PCM = false>
static hipError_t launch_pass2_mc_t(const Pass2Args& a, int n_items, hipStream_t s) {
    const size_t lds = pass2_mc_lds_bytes(C, PCM);
    auto k = beamform_istft_mc_kernel<C, PCM>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(n_items), dim3(p2mc_threads(PCM)), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_pass2_mc(int C, const Pass2Args& a, int n_items, hipStream_t s, bool pcm16) {
#define SETK_CASE(c) \
    case c: return pcm16 ? launch_pass2_mc_t<c, true>(a, n_items, s) : launch_pass2_mc_t<c>(a, n_items, s);
    switch (C) {
        SETK_CASE(1)
        SETK_CASE(2)
        SETK_CASE(3)
        SETK_CASE(4)
        SETK_CASE(5)
        SETK_CASE(6)
        SETK_CASE(7)
        SETK_CASE(8)
    }
#undef SETK_CASE
    return hipErrorInvalidValue;
}

}  // namespace setk
