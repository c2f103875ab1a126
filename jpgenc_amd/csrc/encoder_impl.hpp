// What the Encoder's translation units share (encoder.cpp: the frame pipeline;
// encoder_stripes.cpp: the stripe phases; encoder_planes.cpp: the plane stages).
// Private: included by those three files only.
#pragma once
#include "encoder.hpp"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>

namespace jpge {

#define JPGE_HIP(expr)                                   \
    do {                                                 \
        if ((expr) != hipSuccess) return kErrHip;        \
    } while (0)

// Host-side wait with low wake-up latency (the pipeline waits on short intervals).
hipError_t wait_event(hipEvent_t e);

// Poll a sequence word a kernel writes into mapped host memory after its data
// (release-ordered).  `nap`: sleep ~10 us between polls (pool workers, which have
// slack) instead of spinning (the submitting thread).  Bounded: a stream error or
// ~20 s without progress fails.  The stream is queried only after 2 ms without the
// word (then every ms): a stream query enqueues a marker behind the newest launch,
// which costs the GPU ~6 us of idle each time.  `queued`: set once the kernel that
// writes the word is on the stream (another thread launches it); before that an
// idle stream is no error.
//
// `guess` (napping waits): a running estimate of how long this wait takes at its call
// site.  The first sleep covers most of it in one wake-up, and naps poll the rest, so
// a wait of ~100 us costs two or three wake-ups instead of ten.  The sleep is shortened
// by twice the waits' spread, so irregular waits (16384^2 frames) are polled, not slept
// through.
struct WaitGuess {
    double ema_us = 0;  // smoothed wait duration (0: none yet)
    double dev_us = 0;  // smoothed |wait - ema_us|
    double frac = 0;    // first sleep = frac * ema - 2 * dev (0: off)
    double first_sleep_us() const { return frac * ema_us - 2.0 * dev_us; }
    void add(double us) {
        if (ema_us > 0) {
            dev_us = 0.85 * dev_us + 0.15 * std::fabs(us - ema_us);
            ema_us = 0.85 * ema_us + 0.15 * us;
        } else {
            ema_us = us;
        }
    }
    // statistics (JPGE_CPU_PROF): waits, waits already satisfied on entry, naps, total us
    uint64_t waits = 0, ready = 0, naps = 0;
    double total_us = 0;
};
int wait_seq(const uint64_t* word, uint64_t seq, hipStream_t stream, int nap_us = 0,
             const std::atomic<int>* queued = nullptr, WaitGuess* guess = nullptr,
             const std::function<bool()>* work = nullptr);

// Control block, zeroed at the start of every frame by the first kernel (K1).
struct CtlLayout {
    size_t cnt, key, rec, done, total;  // [0, total): zeroed by K1 every frame
    size_t place, summary, alloc;  // not zeroed (written before they are read)
    explicit CtlLayout(uint32_t ntiles) {  // ntiles: entropy workgroups (records)
        size_t o = 0;
        cnt = o; o += align_up((size_t)kHistReplicas * 4 * 256 * 4, 256);
        key = o; o += align_up(4 * 256 * 8, 256);
        rec = o; o += align_up((size_t)ntiles * kEntropyRecordBytes, 256);
        done = o; o += 256;
        total = o;
        place = o; o += align_up((size_t)ntiles * sizeof(WgPlace), 256);
        summary = o; o += 256;
        alloc = o;
    }
};

struct HostHist {  // written by hist_export_kernel into mapped pinned memory
    uint32_t cnt[4 * 256];  // replicas summed
    uint64_t key[4 * 256];  // ~first-occurrence key
    uint64_t seq;           // frame sequence number, written after the data
};
// an exported histogram as the stage entries return it: the counts, and the
// first-occurrence keys the right way round (absent symbols: all ones)
void read_hist(const HostHist& h, uint32_t counts[1024], uint64_t first[1024]);

// no zero quantiser in either table
bool tables_nonzero(const uint8_t qy[64], const uint8_t qc[64]);

struct Encoder::Slot {
    hipStream_t stream = nullptr;  // the encoder's stream (shared by all slots, not owned)
    // 0-2, 4-5 kernel timing brackets (3, 6, 7 unused)
    hipEvent_t ev[8] = {};
    Geometry g;
    // device workspace (capacities)
    size_t cap_blk = 0, cap_in = 0, cap_out = 0, cap_ctl = 0;
    uint8_t* d_in = nullptr;
    int16_t* d_coef = nullptr;
    uint8_t* d_ctl = nullptr;
    uint8_t* d_ubuf = nullptr;  // unstuffed entropy-coded segment (K3 internal)
    size_t cap_ubuf = 0;
    uint16_t* d_recs = nullptr;    // K2's symbol records, kTileRecords per entropy tile
    uint32_t* d_tcount = nullptr;  // records per tile
    size_t cap_tiles = 0;          // (capacities: records, in words; tiles)
    size_t cap_recs = 0;
    uint8_t* d_out = nullptr;
    uint32_t* d_tab = nullptr;  // [1024] tables, then the header bytes (one upload)
    // pinned host staging
    HostHist* h_hist = nullptr;
    HostHist* d_hist_host = nullptr;  // device view of h_hist
    uint32_t* h_tab = nullptr;     // same layout as d_tab (mapped)
    uint32_t* d_tab_host = nullptr;  // device view of h_tab
    uint64_t* h_result = nullptr;  // mapped: written by the entropy kernel's last workgroup
                                   // ([0, 4)); [6]: encode()'s gate word (gate())
    uint64_t* d_result_host = nullptr;
    // per-frame state between phases (begin() writes it)
    FrameInput in;  // what K1 reads (frame_plan.hpp; a null in.ptr: the slot holds no frame)
    uint8_t* out_dev = nullptr;
    size_t out_cap = 0;
    size_t hdr_len = 0;
    uint64_t symbols = 0;              // Huffman-coded symbols (= K2 symbol records) of the frame
    uint8_t qy[64], qc[64];
    bool timed = false;                // this frame's kernels are bracketed by timing events
    int timed_frames = 1;              // frames those kernels covered (a frame set's launches)
    bool count_symbols = false;        // a member of a timed launch: its symbols go to times_.symbols
    HistPtrs hist{};                   // this frame's device histograms (in d_ctl)
    uint64_t seq = 0;                  // frame sequence number (handshakes via mapped memory)
    std::atomic<int> tables_done{0};   // set by build_tables (any thread)
    std::atomic<int> export_queued{0}; // the kernel exporting this frame's histograms is launched
    std::chrono::steady_clock::time_point t_submit, t_start, t_done;  // table job (host trace)
    // stripe context (a row stripe of a larger image; whole frames: zero seeds and
    // bases, header dimensions = the frame's)
    DcSeed seed;
    Restart rst;  // restart intervals of the frame (stripe: its first MCU in the image's numbering)
    uint64_t key_y0 = 0, key_c0 = 0, key_ncb = 0;
    uint32_t img_w = 0, img_h = 0;
    int tables_status = 0;
    bool inline_tables = false;  // this frame's tables are built inside its lane's pipeline (its waits use the lane's guess)
    // the lane's wait estimates (histograms when its own thread builds the tables; results)
    WaitGuess* guess_hist = nullptr;
    WaitGuess* guess_result = nullptr;
    // Fixed Huffman tables: what h_tab and d_tab hold of them (gen 0: nothing; a frame with
    // per-image tables overwrites both).  A frame whose key equals it finds its code words
    // and headers on the device already.
    struct FixedKey {
        uint64_t gen = 0;  // the setting (Encoder::huff_gen_)
        uint32_t w = 0, h = 0, restart = 0, samp = 0;  // samp: Y sampling (H << 4 | V), 0 = one component
        uint8_t qy[64] = {}, qc[64] = {};
        bool operator==(const FixedKey& o) const {
            return gen == o.gen && w == o.w && h == o.h && restart == o.restart && samp == o.samp &&
                   !std::memcmp(qy, o.qy, 64) && !std::memcmp(qc, o.qc, 64);
        }
    } fixed;

    uint32_t* gate() const { return reinterpret_cast<uint32_t*>(h_result + 6); }

    // Start a frame on the slot: every per-frame field, every time, so nothing is left
    // over from the call that used the slot before (whole frames, stripes and plane sets
    // share lane 0's first slot).  A whole frame: zero DC seeds and key bases, its first
    // MCU the image's, untimed until phase 1 says otherwise.  A stripe then sets its
    // keys and rst.mcu0.  (img_w, img_h: the header's dimensions.)
    void begin(const Geometry& geo, const uint8_t y[64], const uint8_t c[64], const FrameInput& input, uint8_t* out, size_t cap,
               uint32_t restart, uint32_t w, uint32_t h) {
        in = input;
        std::memcpy(qy, y, 64);
        std::memcpy(qc, c, 64);
        g = geo;
        out_dev = out;
        out_cap = cap;
        seed = DcSeed();
        rst = Restart();
        rst.mcus = restart;
        key_y0 = key_c0 = key_ncb = 0;
        img_w = w;
        img_h = h;
        timed = false;
        timed_frames = 1;
        count_symbols = false;
        tables_done.store(0, std::memory_order_relaxed);
        export_queued.store(0, std::memory_order_relaxed);
    }

    // The carried export of `e`: its code kernel takes exp's histograms (a later frame's)
    // to the host on the way; nullptr: none.
    static void carry_export(EntropyArgs& e, const Slot* exp) {
        e.exp_hist = exp ? exp->hist : HistPtrs{};
        e.exp_cnt = exp ? exp->d_hist_host->cnt : nullptr;
        e.exp_key = exp ? exp->d_hist_host->key : nullptr;
        e.exp_seq = exp ? &exp->d_hist_host->seq : nullptr;
        e.exp_seqv = exp ? exp->seq : 0;
    }

    ~Slot() {
        hipFree(d_in); hipFree(d_coef); hipFree(d_ctl); hipFree(d_ubuf);
        hipFree(d_recs); hipFree(d_tcount);
        hipFree(d_out); hipFree(d_tab);
        hipHostFree(h_hist); hipHostFree(h_tab); hipHostFree(h_result);
        for (auto& e : ev) if (e) hipEventDestroy(e);
    }
};

}  // namespace jpge
