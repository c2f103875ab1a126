#include "encoder_impl.hpp"
#include "host_par.hpp"

#include <algorithm>
#include <array>
#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <mutex>
#include <string>
#include <thread>

#include <sys/prctl.h>
#include <vector>

namespace jpge {

// (encoder_impl.hpp describes both waits)
hipError_t wait_event(hipEvent_t e) {
    hipError_t r;
    while ((r = hipEventQuery(e)) == hipErrorNotReady) {
    }
    return r;
}
int wait_seq(const uint64_t* word, uint64_t seq, hipStream_t stream, int nap_us, const std::atomic<int>* queued,
             WaitGuess* guess, const std::function<bool()>* work) {
    const bool nap = nap_us > 0;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    auto next_query = t0 + std::chrono::milliseconds(2);
    clk::time_point idle_since{};  // the stream was first seen idle without the word
    bool idle = false;
    if (guess) ++guess->waits;
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) {  // (not a wait: the estimate is of waits)
        if (guess) ++guess->ready;
        return kOk;
    }
    // (idle work first: the first sleep only once there is none)
    bool worked = false;
    while (work && __atomic_load_n(word, __ATOMIC_ACQUIRE) != seq && (*work)()) worked = true;
    if (nap && guess && guess->frac > 0 && !worked) {
        const double us = guess->first_sleep_us();
        if (us > 3.0 * nap_us) {
            std::this_thread::sleep_for(std::chrono::microseconds((long)us));
            ++guess->naps;
        }
    }
    for (uint32_t spins = 0;; ++spins) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) {
            if (guess) {
                const double us = std::chrono::duration<double, std::micro>(clk::now() - t0).count();
                guess->add(us);
                guess->total_us += us;
            }
            return kOk;
        }
        if (work && (*work)()) continue;
        if (nap) {
            std::this_thread::sleep_for(std::chrono::microseconds(nap_us));
            if (guess) ++guess->naps;
        }
        if (!nap && (spins & 255) != 255) continue;
        const auto now = clk::now();
        if (now < next_query) continue;
        next_query = now + std::chrono::milliseconds(1);
        const hipError_t q = hipStreamQuery(stream);
        if (q != hipSuccess && q != hipErrorNotReady) return kErrHip;
        // An idle stream without the word: its writer never ran (an error), or the
        // word is still on its way to host memory (seen with several processes on one
        // GPU): an error only once it stays missing for 200 ms.
        if (q == hipSuccess && __atomic_load_n(word, __ATOMIC_ACQUIRE) != seq &&
            (!queued || queued->load(std::memory_order_acquire))) {
            if (!idle) {
                idle = true;
                idle_since = now;
            } else if (now - idle_since > std::chrono::milliseconds(200)) {
                if (std::getenv("JPGE_DEBUG")) std::fprintf(stderr, "jpge: wait_seq: word %llu != %llu, stream idle\n",
                                                          (unsigned long long)__atomic_load_n(word, __ATOMIC_ACQUIRE),
                                                          (unsigned long long)seq);
                return kErrInternal;
            }
        } else {
            idle = false;
        }
        if (now - t0 > std::chrono::seconds(20)) return kErrTimeout;
    }
}

void read_hist(const HostHist& h, uint32_t counts[1024], uint64_t first[1024]) {
    for (int i = 0; i < 1024; ++i) {
        counts[i] = h.cnt[i];
        first[i] = h.cnt[i] ? ~h.key[i] : ~0ull;
    }
}

bool tables_nonzero(const uint8_t qy[64], const uint8_t qc[64]) {
    for (int i = 0; i < 64; ++i)
        if (!qy[i] || !qc[i]) return false;
    return true;
}

namespace {

// Pipeline depth limits (defaults in Encoder; the slots in flight = lookahead + drain lag + 1).
constexpr int kMaxLookahead = 8;
constexpr int kMaxDrainLag = 4;
constexpr int kMaxLanes = 8;
constexpr uint64_t kFirstSleepMaxPixels = 16u << 20;   // frames this large poll their results without a first sleep

double abs_us(std::chrono::steady_clock::time_point t) {  // host-trace clock
    return std::chrono::duration<double, std::micro>(t.time_since_epoch()).count();
}

int env_int(const char* name, int dflt, int lo, int hi) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    const long x = std::strtol(v, nullptr, 10);
    return x < lo ? lo : x > hi ? hi : (int)x;
}

int64_t thread_cpu_ns() {  // the calling thread's CPU time (JPGE_CPU_PROF)
    timespec t;
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t);
    return (int64_t)t.tv_sec * 1000000000 + t.tv_nsec;
}

constexpr size_t kTabBytes = 4 * 256 * 4;  // code tables as uploaded
constexpr size_t kHdrMax = 4096;           // headers SOI .. SOS (<= 20 + 2*69 + 19 + 4*277 + 14)

constexpr size_t kStatsDoneOff = 64;  // K2's finished-workgroup count: a line of its own in the `done` block
constexpr size_t kPackDoneOff = 128;  // the pack kernel's count, end offset and flag: another line

}  // namespace

// A 1-lane encoder's second table thread, for single images (encode()): while the calling
// thread builds the luma AC table (the largest: ~2/3 of a frame's table time), it builds
// the other three.  It is armed when a call starts waiting for its histograms (so its
// wake-up overlaps the two kernels), spins only until the call's tables are built, and
// otherwise sleeps on a condition variable.
class Encoder::TableHelper {
  public:
    TableHelper() {
        th_ = std::thread([this] {
            prctl(PR_SET_NAME, "jpge-tables", 0, 0, 0);
            run();
        });
    }
    ~TableHelper() {
        state_.store(kStop, std::memory_order_release);
        { std::lock_guard<std::mutex> g(mu_); }
        cv_.notify_one();
        th_.join();
    }
    void arm() {
        int idle = kIdle;
        if (state_.compare_exchange_strong(idle, kArmed, std::memory_order_acq_rel)) {
            { std::lock_guard<std::mutex> g(mu_); }
            cv_.notify_one();
        }
    }
    void disarm() {
        int s = state_.load(std::memory_order_acquire);
        while ((s == kArmed || s == kDone) && !state_.compare_exchange_weak(s, kIdle, std::memory_order_acq_rel)) {
        }
    }
    // tables 0, 2 and 3 (DC luma, DC and AC chroma) on the helper; false: not armed (the
    // caller builds them itself)
    bool post(const uint32_t* cnt, const uint64_t* key, bool inverted, HuffTable* tabs, int* ok) {
        if (state_.load(std::memory_order_acquire) != kArmed) return false;
        cnt_ = cnt;
        key_ = key;
        inv_ = inverted;
        tabs_ = tabs;
        ok_ = ok;
        int armed = kArmed;
        return state_.compare_exchange_strong(armed, kJob, std::memory_order_acq_rel);
    }
    void wait() {
        while (state_.load(std::memory_order_acquire) != kDone) __builtin_ia32_pause();
    }

  private:
    enum { kIdle, kArmed, kJob, kDone, kStop };
    void run() {
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return state_.load(std::memory_order_acquire) != kIdle; });
            }
            for (;;) {
                const int s = state_.load(std::memory_order_acquire);
                if (s == kStop) return;
                if (s == kIdle) break;
                if (s == kJob) {
                    for (int t : {0, 2, 3})
                        ok_[t] = inv_ ? build_table_inverted(cnt_ + t * 256, key_ + t * 256, tabs_[t])
                                      : build_table(cnt_ + t * 256, key_ + t * 256, tabs_[t]);
                    state_.store(kDone, std::memory_order_release);
                    continue;
                }
                __builtin_ia32_pause();
            }
        }
    }
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::atomic<int> state_{kIdle};
    const uint32_t* cnt_ = nullptr;
    const uint64_t* key_ = nullptr;
    bool inv_ = false;
    HuffTable* tabs_ = nullptr;
    int* ok_ = nullptr;
};

// An independent pipeline: its own stream and slot ring; lanes other than 0 own a
// host thread that runs the lane's share of a batch.  Between batches the thread
// polls for ~1 ms (back-to-back batches start without a wake-up), then blocks.
struct Encoder::Lane {
    int id = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;  // end of the lane's batch work on its stream
    std::vector<std::unique_ptr<Slot>> slots;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    int result = 0;
    std::atomic<uint32_t> posted{0}, finished{0};
    std::atomic<bool> stop{false};
    WaitGuess guess_hist, guess_result;  // (the slots point here)

    void start() {
        th = std::thread([this] {
            prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
            const std::string name = "jpge-lane" + std::to_string(id);
            prctl(PR_SET_NAME, name.c_str(), 0, 0, 0);
            uint32_t seen = 0;
            for (;;) {
                const auto t0 = std::chrono::steady_clock::now();
                while (posted.load(std::memory_order_acquire) == seen && !stop.load(std::memory_order_acquire)) {
                    if (std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(1)) {
                        std::this_thread::yield();
                        continue;
                    }
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return posted.load(std::memory_order_acquire) != seen || stop.load(); });
                }
                if (posted.load(std::memory_order_acquire) == seen) return;  // stopped
                seen = posted.load(std::memory_order_acquire);
                result = job();
                finished.store(seen, std::memory_order_release);
            }
        });
    }
    void post(std::function<int()> f) {
        job = std::move(f);
        posted.fetch_add(1, std::memory_order_acq_rel);
        { std::lock_guard<std::mutex> g(mu); }
        cv.notify_one();
    }
    int wait() {
        const uint32_t want = posted.load(std::memory_order_acquire);
        while (finished.load(std::memory_order_acquire) != want) std::this_thread::yield();
        return result;
    }
    void shutdown() {
        if (!th.joinable()) return;
        stop.store(true, std::memory_order_release);
        { std::lock_guard<std::mutex> g(mu); }
        cv.notify_one();
        th.join();
    }
};

int Encoder::set_restart(uint32_t mcus) {
    if (mcus > 65535) return kErrArg;  // DRI carries a 16-bit interval
    restart_mcus_ = mcus;
    return kOk;
}

int Encoder::set_input_format(int fmt, size_t plane_stride) {
    if (!fmt_valid(fmt)) return kErrArg;
    if (plane_stride && fmt_planes(fmt) == 1) return kErrArg;
    fmt_ = fmt;
    plane_stride_ = plane_stride;
    return kOk;
}

int Encoder::set_downscale(int factor) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    if (!ds_valid(factor)) return kErrArg;
    ds_ = factor;
    return kOk;
}

int Encoder::downscale() {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    return ds_;
}

int Encoder::set_orientation(int o) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    if (!orient_valid(o)) return kErrArg;
    orient_ = o;
    return kOk;
}

int Encoder::orientation() {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    return orient_;
}

int Encoder::set_channel_lut(const uint8_t* lut) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    if (!lut) {
        lut_on_ = false;
        return kOk;
    }
    // (the call holds the context: no frame is in flight, so the one device copy can be rewritten;
    // on a stream of the context's own, and awaited: every lane's next launch sees the new bytes,
    // and the caller's buffer and lut_ are free to change)
    JPGE_HIP(hipSetDevice(device_));
    if (!d_lut_) JPGE_HIP(hipMalloc((void**)&d_lut_, kLutBytes));
    lut_on_ = false;  // (a failed upload leaves the tables off, not half written and on)
    std::memcpy(lut_, lut, kLutBytes);
    hipStream_t stream = lanes_[0]->stream;
    JPGE_HIP(hipMemcpyAsync(d_lut_, lut_, kLutBytes, hipMemcpyHostToDevice, stream));
    JPGE_HIP(hipStreamSynchronize(stream));
    lut_on_ = true;
    return kOk;
}

void Encoder::channel_lut(int* on, uint8_t* lut) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    if (on) *on = lut_on_ ? 1 : 0;
    if (lut) std::memcpy(lut, lut_, kLutBytes);
}

int Encoder::set_yuv_transform(int preset, const YuvXf* custom) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    YuvXf t;
    if (const int st = yuv_setting_check(preset, custom, t)) return st;
    yuv_preset_ = preset;
    yuv_xf_ = t;
    return kOk;
}

void Encoder::yuv_transform(int* preset, YuvXf* t) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    if (preset) *preset = yuv_preset_;
    if (t) *t = yuv_xf_;
}

int Encoder::set_subsampling(int mode) {
    uint32_t yh, bpm, cf;
    if (!mode_shape(mode, yh, bpm, cf)) return kErrArg;
    mode_ = mode;
    return kOk;
}

int Encoder::set_huffman(int mode, const HuffSpec* specs) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    if (const int st = huff_setting_check(mode, specs)) return st;
    if (mode) {
        // the code words once, here: no frame of this setting builds a table
        const HuffSpec* src = mode == 1 ? kAnnexKHuffman : specs;
        for (int t = 0; t < 4; ++t) {
            huff_specs_[t] = src[t];
            huff_spec_table(huff_specs_[t], huff_tabs_[t]);
            for (int i = 0; i < 256; ++i)
                huff_words_[t * 256 + i] = ((uint32_t)huff_tabs_[t].len[i] << 16) | (huff_tabs_[t].code[i] & 0xFFFF);
        }
        ++huff_gen_;
    }
    huff_mode_ = mode;
    return kOk;
}

void Encoder::huffman(int* mode, HuffSpec* specs) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    if (mode) *mode = huff_mode_;
    if (specs && huff_mode_)
        for (int t = 0; t < 4; ++t) specs[t] = huff_specs_[t];
}

// A frame's code words and headers in a fixed mode.  The headers depend on the frame's
// size, quantisers, sampling and restart interval and on the tables, all known when the
// frame is queued; a slot that coded such a frame last keeps them, on the host and on the
// device (a lane's steady state on one geometry writes neither).
int Encoder::fixed_tables(Slot& s, bool& fresh) {
    const bool gray = s.g.gray();
    Slot::FixedKey k;
    k.gen = huff_gen_;
    k.w = s.img_w;
    k.h = s.img_h;
    k.restart = s.rst.mcus;
    k.samp = gray ? 0u : (s.g.yh << 4) | s.g.yv();
    std::memcpy(k.qy, s.qy, 64);
    std::memcpy(k.qc, s.qc, 64);
    s.symbols = 0;  // (counted from the histograms, which a fixed mode does not have)
    fresh = !(k == s.fixed);
    if (fresh) {
        s.fixed.gen = 0;
        std::memcpy(s.h_tab, huff_words_, kTabBytes);
        // (one component: the chroma tables' slots stay unused, zeroed as build_tables_from leaves them)
        if (gray) std::memset(s.h_tab + 2 * 256, 0, 2 * 256 * sizeof(uint32_t));
        const HuffTable* tp[4] = {&huff_tabs_[0], &huff_tabs_[1], &huff_tabs_[2], &huff_tabs_[3]};
        const std::vector<uint8_t> hdr = gray ? jfif_headers_gray(s.img_w, s.img_h, s.qy, tp, s.rst.mcus)
                                              : jfif_headers(s.img_w, s.img_h, s.qy, s.qc, tp, s.rst.mcus,
                                                             (uint8_t)k.samp);
        if (hdr.size() > kHdrMax) return kErrInternal;
        std::memcpy(reinterpret_cast<uint8_t*>(s.h_tab) + kTabBytes, hdr.data(), hdr.size());
        s.hdr_len = hdr.size();
        s.fixed = k;
    }
    if (s.out_cap && s.out_cap < s.hdr_len + 2) return kErrNoSpace;
    return kOk;
}

size_t Encoder::max_jpeg_bytes(uint32_t w, uint32_t h) { return jpge::max_jpeg_bytes(w, h); }

int Encoder::open(int device, std::unique_ptr<Encoder>& out, int lanes) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return kErrNoDevice;
    if (device < 0 || device >= n) return kErrNoDevice;
    JPGE_HIP(hipSetDevice(device));
    std::unique_ptr<Encoder> e(new Encoder());
    e->device_ = device;
    if (const char* ew = std::getenv("JPGE_ENTROPY_WGS")) e->entropy_wgs_ = (uint32_t)std::strtoul(ew, nullptr, 10);
    if (const char* sw = std::getenv("JPGE_STATS_WGS")) e->stats_wgs_ = (uint32_t)std::strtoul(sw, nullptr, 10);
    e->fdct_wgs_ = (uint32_t)env_int("JPGE_FDCT_WGS", 0, 0, 65536);
    e->stamps_file_ = std::getenv("JPGE_STAMPS_FILE");
    e->host_trace_file_ = std::getenv("JPGE_HOST_TRACE");
    e->cpu_prof_ = env_int("JPGE_CPU_PROF", 0, 0, 1) != 0;
    e->lat_prof_ = env_int("JPGE_LAT_PROF", 0, 0, 1) != 0;
    e->table_helper_ = env_int("JPGE_TABLE_HELPER", 1, 0, 1) != 0;
    e->gate_ = env_int("JPGE_GATE", 1, 0, 2);
    // Launch-serialising debug modes block the host in a launch until the kernel (or its
    // predecessor) has finished, so the host could never open the gate behind the gate
    // kernel: every call would run into its time-out.  They get the ungated path.
    if (env_int("AMD_SERIALIZE_KERNEL", 0, 0, 3) != 0 || env_int("HIP_LAUNCH_BLOCKING", 0, 0, 1) != 0) e->gate_ = 0;
    if (const int us = env_int("JPGE_TEST_GATE_TIMEOUT_US", 0, 0, 1000000)) e->gate_ticks_ = 100ull * (uint64_t)us;
    e->gate_delay_us_ = env_int("JPGE_TEST_GATE_DELAY_US", 0, 0, 1000000);
    if (e->gate_ == 2) {  // (the runtime's stream wait needs device support)
        int wv = 0;
        if (hipDeviceGetAttribute(&wv, hipDeviceAttributeCanUseStreamWaitValue, device) != hipSuccess || !wv) e->gate_ = 0;
        (void)hipGetLastError();
    }
    e->hist_nap_us_ = env_int("JPGE_HIST_NAP_US", e->hist_nap_us_, 0, 1000);
    e->lookahead_ = env_int("JPGE_LOOKAHEAD", e->lookahead_, 1, kMaxLookahead);
    e->drain_lag_ = env_int("JPGE_DRAIN_LAG", e->drain_lag_, 0, kMaxDrainLag);
    e->set_ = env_int("JPGE_SET", 0, 0, kMaxSet);
    e->nap_us_ = env_int("JPGE_NAP_US", e->nap_us_, 1, 1000);
    e->first_sleep_ = env_int("JPGE_FIRST_SLEEP", (int)(e->first_sleep_ * 100 + 0.5), 0, 95) / 100.0;
    const int nap = env_int("JPGE_NAP", -1, -1, 1);
    e->ext_place_ = env_int("JPGE_EXT_PLACE", -1, -1, 1);
    e->place_in_code_ = env_int("JPGE_PLACE_IN_CODE", 1, 0, 1) != 0;
    if (e->stamps_file_) {
        e->dbg_words_ = 4ull * 65536 * kStampSlots;  // up to 64k workgroups per kernel, 4 kernels
        JPGE_HIP(hipMalloc((void**)&e->d_dbg_, e->dbg_words_ * 8));
        JPGE_HIP(hipMemset(e->d_dbg_, 0, e->dbg_words_ * 8));  // (diagnostic stamps only: the null stream)
    }
    // Lanes: each an in-order stream whose frame i+1.. transform and statistics
    // kernels are queued ahead of frame i's entropy kernels, so the host builds frame
    // i's tables while the GPU works on later frames.  Lanes run frames side by side,
    // so one lane's kernels fill another's launch tails and latency-bound phases
    // (4 lanes = the hardware queues HIP opens per process; measured best).
    const int nlanes = e->stamps_file_ ? 1
                       : lanes > 0   ? std::min(lanes, kMaxLanes)
                                     : env_int("JPGE_LANES", 4, 1, kMaxLanes);
    // Lane threads nap between polls when several lanes share the GPU: the same
    // throughput at 2.6 instead of 5.8 host CPUs per GPU (4 lanes, 4K bench); a single
    // lane spins for its latency.
    e->nap_ = nap < 0 ? nlanes > 1 : nap != 0;
    const int nslots = e->lookahead_ + e->drain_lag_ + 1;  // a slot is reused after its drain
    // Several lanes: each lane's stream is created with a full CU mask, which gives it a
    // hardware queue of its own (ROCclr hands such a stream a dedicated queue instead of
    // one from the process's shared pool of GPU_MAX_HW_QUEUES).  From the pool, two lanes
    // could land on one in-order queue and serialise: the 1080p batch (config 4) ran
    // 107.8-109.9 vs 88.6-90.8 GPix/s, the same as with GPU_MAX_HW_QUEUES=6 (110.2-110.3);
    // 4K unchanged (185.2 vs 185.4).  JPGE_CU_MASK_STREAMS=0: pool streams.
    const bool cumask = env_int("JPGE_CU_MASK_STREAMS", nlanes > 1 ? 1 : 0, 0, 1) != 0;
    std::vector<uint32_t> mask;
    if (cumask) {
        int ncu = 0;
        JPGE_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
        mask.assign((size_t)(ncu + 31) / 32, 0xFFFFFFFFu);
        if (ncu % 32) mask.back() = (1u << (ncu % 32)) - 1u;
    }
    for (int l = 0; l < nlanes; ++l) {
        std::unique_ptr<Lane> ln(new Lane());
        ln->id = l;
        // (a runtime that refuses CU masks gets a pool stream: correct, possibly shared)
        if (!cumask || hipExtStreamCreateWithCUMask(&ln->stream, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            JPGE_HIP(hipStreamCreateWithFlags(&ln->stream, hipStreamNonBlocking));
        }
        JPGE_HIP(hipEventCreateWithFlags(&ln->done, hipEventDisableTiming));
        ln->guess_hist.frac = ln->guess_result.frac = e->first_sleep_;
        if (const int st = e->add_slots(*ln, nslots)) return st;
        if (l > 0) ln->start();
        e->lanes_.push_back(std::move(ln));
    }
    out = std::move(e);
    return kOk;
}

int Encoder::add_slots(Lane& ln, int count) {
    while ((int)ln.slots.size() < count) {
        std::unique_ptr<Slot> s(new Slot());
        s->stream = ln.stream;
        s->guess_hist = &ln.guess_hist;
        s->guess_result = &ln.guess_result;
        for (int k = 0; k < 8; ++k)
            JPGE_HIP(hipEventCreateWithFlags(&s->ev[k], hipEventDefault));
        JPGE_HIP(hipHostMalloc((void**)&s->h_hist, sizeof(HostHist), hipHostMallocMapped));
        JPGE_HIP(hipHostGetDevicePointer((void**)&s->d_hist_host, s->h_hist, 0));
        JPGE_HIP(hipHostMalloc((void**)&s->h_tab, kTabBytes + kHdrMax, hipHostMallocMapped));
        JPGE_HIP(hipHostGetDevicePointer((void**)&s->d_tab_host, s->h_tab, 0));
        // (zeroed: a code kernel behind encode()'s gate reads whatever tables are here when
        // a table build fails, and zero lengths keep it within its bounds)
        std::memset(s->h_tab, 0, kTabBytes + kHdrMax);
        JPGE_HIP(hipHostMalloc((void**)&s->h_result, 64, hipHostMallocMapped));
        std::memset(s->h_result, 0, 64);
        JPGE_HIP(hipHostGetDevicePointer((void**)&s->d_result_host, s->h_result, 0));
        JPGE_HIP(hipMalloc((void**)&s->d_tab, kTabBytes + kHdrMax));
        // (zeroed too: a gate that times out leaves the code kernel these tables, ADVICE r5;
        // on the lane's stream: an operation on the null stream made every later launch on
        // the lanes' streams slower, the 4K pipeline -3%)
        JPGE_HIP(hipMemsetAsync(s->d_tab, 0, kTabBytes + kHdrMax, ln.stream));
        ln.slots.push_back(std::move(s));
    }
    return kOk;
}

Encoder::~Encoder() {
    if (lat_prof_ && lat_calls_)
        std::fprintf(stderr, "jpge encode() phases per call (us, wall): launch-1 %.2f histogram-wait %.2f tables %.2f "
                             "launch-entropy %.2f result-wait %.2f end %.2f (%lld calls)\n",
                     lat_ns_[0] / 1e3 / lat_calls_, lat_ns_[1] / 1e3 / lat_calls_, lat_ns_[2] / 1e3 / lat_calls_,
                     lat_ns_[3] / 1e3 / lat_calls_, lat_ns_[4] / 1e3 / lat_calls_, lat_ns_[5] / 1e3 / lat_calls_,
                     (long long)lat_calls_);
    if (lat_prof_ && lat_calls_)
        std::fprintf(stderr, "jpge   of launch-1: argument preparation %.2f, K1 launch %.2f\n", lat_ns_[6] / 1e3 / lat_calls_,
                     lat_ns_[7] / 1e3 / lat_calls_);
    if (cpu_prof_ && cpu_frames_.load()) {
        const double f = (double)cpu_frames_.load();
        std::fprintf(stderr, "jpge cpu per frame (us): tables %.2f launch-1 %.2f launch-entropy %.2f finish %.2f "
                             "loop-top %.2f end %.2f\n",
                     cpu_ns_[1] / f / 1e3, cpu_ns_[2] / f / 1e3, cpu_ns_[3] / f / 1e3, cpu_ns_[4] / f / 1e3,
                     cpu_ns_[0] / f / 1e3, cpu_ns_[5] / f / 1e3);
        if (cpu_builds_.load())
            std::fprintf(stderr, "jpge table builds: %lld, histogram read %.2f us, tables + headers %.2f us each\n",
                         (long long)cpu_builds_.load(), cpu_read_ns_.load() / 1e3 / cpu_builds_.load(),
                         cpu_build_ns_.load() / 1e3 / cpu_builds_.load());
        if (cpu_builds_.load())
            std::fprintf(stderr, "jpge   of which: 4 tables %.2f us, code words to mapped memory %.2f us, headers %.2f us\n",
                         cpu_part_ns_[0].load() / 1e3 / cpu_builds_.load(), cpu_part_ns_[1].load() / 1e3 / cpu_builds_.load(),
                         cpu_part_ns_[2].load() / 1e3 / cpu_builds_.load());
        for (auto& ln : lanes_)
            for (const WaitGuess* g : {&ln->guess_hist, &ln->guess_result})
                std::fprintf(stderr, "jpge lane %d %s waits: %llu (%llu ready on entry), %.2f naps and %.1f us per wait, ema %.1f\n",
                             ln->id, g == &ln->guess_hist ? "histogram" : "result", (unsigned long long)g->waits,
                             (unsigned long long)g->ready, g->waits ? (double)g->naps / g->waits : 0.0,
                             g->waits ? g->total_us / g->waits : 0.0, g->ema_us);
    }
    helper_.reset();
    for (auto& ln : lanes_) ln->shutdown();
    for (auto& b : scratch_) hipFree(b.first);
    hipSetDevice(device_);
    for (auto& ln : lanes_) {
        if (ln->stream) hipStreamSynchronize(ln->stream);
        ln->slots.clear();
        if (ln->done) hipEventDestroy(ln->done);
        if (ln->stream) hipStreamDestroy(ln->stream);
    }
    hipFree(d_dbg_);
    hipFree(d_lut_);
}

// Diagnostic: raw per-workgroup phase stamps of the last frame, as
// [u64 n_fdct_wg, n_stats_wg, n_code_wg, n_pack_wg] then 4 x 65536 x kStampSlots u64;
// the buffer is cleared afterwards (slots 8-15 accumulate).
void Encoder::dump_stamps(const Slot& s) {
    if (!stamps_file_ || !d_dbg_) return;
    std::vector<uint64_t> h(dbg_words_);
    if (hipMemcpy(h.data(), d_dbg_, dbg_words_ * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    const uint64_t hdr[4] = {fdct_grid(s.g, lanes_.size() == 1, fdct_wgs_), stats_grid(layout(s.g), stats_wgs()), layout(s.g).grid(),
                             layout(s.g).grid()};
    FILE* f = std::fopen(stamps_file_, "wb");
    if (!f) return;
    std::fwrite(hdr, 8, 4, f);
    std::fwrite(h.data(), 8, h.size(), f);
    std::fclose(f);
    hipMemset(d_dbg_, 0, dbg_words_ * 8);
}

// A workspace buffer of at least `need` units (`bytes` for them): kept, or freed and
// allocated anew.  After a failed allocation the pointer is null and the capacity zero.
template <class T>
static int grow(T*& p, size_t& cap, size_t need, size_t bytes) {
    if (need <= cap) return kOk;
    hipFree(p);
    p = nullptr;
    cap = 0;
    JPGE_HIP(hipMalloc((void**)&p, bytes));
    cap = need;
    return kOk;
}

int Encoder::ensure(Slot& s, const Geometry& g, size_t in_bytes, size_t out_cap) {
    const size_t nblk = g.nblocks();
    if (const int st = grow(s.d_coef, s.cap_blk, nblk, nblk * 128)) return st;
    const CtlLayout L(layout(g).grid());
    const size_t ntiles = seg_tiles(layout(g));
    const size_t nrecs = ntiles * kTileRecords;
    if (ntiles > s.cap_tiles || nrecs > s.cap_recs) {  // (the records and their counts grow together)
        s.cap_tiles = s.cap_recs = 0;
        if (const int st = grow(s.d_recs, s.cap_recs, nrecs, nrecs * sizeof(*s.d_recs))) return st;
        if (const int st = grow(s.d_tcount, s.cap_tiles, ntiles, ntiles * kRecSub * 4)) return st;
    }
    const size_t ubuf = entropy_ubuf_bytes(layout(g));
    if (const int st = grow(s.d_ubuf, s.cap_ubuf, ubuf, ubuf)) return st;
    if (const int st = grow(s.d_ctl, s.cap_ctl, L.alloc, L.alloc)) return st;
    if (const int st = grow(s.d_in, s.cap_in, in_bytes, in_bytes)) return st;
    return grow(s.d_out, s.cap_out, out_cap, out_cap);
}

SegLayout Encoder::slot_layout(const Slot& s) const {
    return seg_layout(s.g, s.rst.mcus, entropy_wgs());
}

// Kernel parameter blocks of a slot's frame (or stripe).
FdctArgs Encoder::fdct_args(Slot& s, int maxval, Slot* imp) {
    const CtlLayout L(slot_layout(s).grid());
    FdctArgs a;
    a.rgb = s.in.ptr;
    a.stride = s.in.stride;
    a.fmt = s.in.fmt;
    a.plane_stride = s.in.plane_stride;
    a.ds = (uint32_t)s.in.ds;
    a.orient = (uint32_t)s.in.orient;
    a.src_w = s.in.src_w;
    a.src_h = s.in.src_h;
    // the sample transform of Y, Cb, Cr and gray frames (FULL_601: the kExact instances)
    // (10-bit samples always: FULL_601 runs it with the identity, for its clamps)
    a.xf_on = ((fmt_yuv(s.in.fmt) || fmt_gray(s.in.fmt)) && yuv_preset_ != kYuvFull601) || fmt_yuv10(s.in.fmt) ? 1u : 0u;
    if (a.xf_on) {
        a.xf[0] = yuv_xf_.y_off;
        for (int i = 0; i < 7; ++i) a.xf[1 + i] = yuv_xf_.m[i];
    }
    // the channel tables (plan_frame has refused the frames that have no such kernel)
    if (lut_on_ && lut_fmt(s.in.fmt)) fdct_set_lut(a, d_lut_);
    a.g = s.g;
    a.maxval = maxval;
    a.solo = lanes_.size() == 1;  // (several lanes: K1 runs beside other frames' kernels)
    a.wgs = fdct_wgs_;
    for (int i = 0; i < 64; ++i) {
        a.q[i] = s.qy[i];
        a.q[64 + i] = s.qc[i];
    }
    a.coef = s.d_coef;
    a.zero = reinterpret_cast<uint32_t*>(s.d_ctl);
    a.zero_words = (uint32_t)(L.total / 4);
    a.imp_src = imp ? reinterpret_cast<const uint4*>(imp->d_tab_host) : nullptr;
    a.imp_dst = imp ? reinterpret_cast<uint4*>(imp->d_tab) : nullptr;
    a.imp_n16 = imp ? (uint32_t)((kTabBytes + imp->hdr_len + 15) / 16) : 0u;
    a.dbg = d_dbg_;
    return a;
}

StatsArgs Encoder::stats_args(Slot& s) {
    const CtlLayout L(slot_layout(s).grid());
    StatsArgs st;
    st.coef = s.d_coef;
    st.g = s.g;
    st.hist.cnt = reinterpret_cast<uint32_t*>(s.d_ctl + L.cnt);
    st.hist.key = reinterpret_cast<uint64_t*>(s.d_ctl + L.key);
    st.seed = s.seed;
    st.rst = s.rst;
    st.key_y0 = s.key_y0;
    st.key_c0 = s.key_c0;
    st.key_ncb = s.key_ncb;
    st.seg = seg_layout(s.g, s.rst.mcus, entropy_wgs());
    st.recs = s.d_recs;
    st.tcount = s.d_tcount;
    st.wgs = stats_wgs();
    if (!stats_wgs_ && lanes_.size() > 1) {
        // frames under ~3 MPix (fewer than 3 tiles per workgroup at 384): about 3 tiles per
        // workgroup, not one each (a workgroup's fixed costs, its first load not overlapped:
        // 1080p batch +9%); 4K and larger keep one workgroup per CU (stats_wgs)
        const uint32_t t = seg_tiles(st.seg);
        if (t < 3u * 384u) st.wgs = std::max(1u, (t + 2) / 3);
    }
    st.dbg = d_dbg_ ? d_dbg_ + 65536 * kStampSlots : nullptr;
    return st;
}

EntropyArgs Encoder::entropy_args(Slot& s) {
    const CtlLayout L(slot_layout(s).grid());
    EntropyArgs e;
    e.coef = s.d_coef;
    e.recs = s.d_recs;
    e.tcount = s.d_tcount;
    e.g = s.g;
    e.tables = s.d_tab;
    e.out = s.out_dev;
    e.hdr_len = s.hdr_len;
    e.out_cap = s.out_cap;
    e.rec = s.d_ctl + L.rec;
    e.place = reinterpret_cast<WgPlace*>(s.d_ctl + L.place);
    e.summary = reinterpret_cast<StripeSummary*>(s.d_ctl + L.summary);
    if (ext_place_ > 0 || (ext_place_ < 0 && lanes_.size() > 1)) {
        e.flags |= kExtPlace;
        // the last code workgroup places every workgroup (no placement launch); the
        // counter is in the block K1 zeroes
        if (place_in_code_ && !s.rst.mcus && slot_layout(s).grid() <= kPlaceInCodeMaxWgs)
            e.done = reinterpret_cast<uint32_t*>(s.d_ctl + L.done);
    }
    e.host_result = s.d_result_host;
    e.seq = s.seq;
    e.ubuf = s.d_ubuf;
    e.wgs = entropy_wgs_;
    e.seed = s.seed;
    e.rst = s.rst;
    e.seg = slot_layout(s);
    if (s.rst.mcus) {  // a stripe's first interval follows the previous stripes' ones
        e.seg_index0 = s.rst.mcu0 / s.rst.mcus;
        e.seg_markers0 = e.seg_index0 > 0 ? 1u : 0u;
    }
    Slot::carry_export(e, nullptr);
    e.dbg = d_dbg_ ? d_dbg_ + 2 * 65536 * kStampSlots : nullptr;
    return e;
}

// Phase 1's host half: the plan (every refusal but the quantisers', before a slot grows or
// anything is queued), the upload of a host frame, the slot's state and the kernels' arguments.
int Encoder::prep1(Slot& s, const FrameDesc& f, const uint8_t qy[64], const uint8_t qc[64], uint32_t flags,
                   Slot* imp, FdctArgs& a, StatsArgs& st) {
    FramePlan p;
    if (const int st0 = plan_frame(f, plan_settings(), flags, p)) return st0;
    if (p.g.gray()) qc = qy;  // (one component: qc is not read)
    if (!tables_nonzero(qy, qc)) return kErrArg;
    if (const int st0 = ensure(s, p.g, p.in_bytes, p.out_cap)) return st0;
    if (p.linear) JPGE_HIP(hipMemcpyAsync(s.d_in, f.rgb, p.linear, hipMemcpyHostToDevice, s.stream));
    for (int c = 0; c < p.ncopy; ++c) {
        const CopyRect& r = p.copy[c];
        JPGE_HIP(hipMemcpy2DAsync(s.d_in + r.dst_off, r.dst_pitch, f.rgb + r.src_off, r.src_pitch, r.row_bytes, r.rows,
                                  hipMemcpyHostToDevice, s.stream));
    }
    if (!p.in.ptr) p.in.ptr = s.d_in;  // (a host frame: K1 reads the copy)
    const bool dev_out = (flags & kFlagDeviceOutput) != 0;
    s.begin(p.g, qy, qc, p.in, dev_out ? f.out : s.d_out, dev_out ? f.cap : s.cap_out, restart_mcus_, p.g.width, p.g.height);
    if (flags & kFlagFixedTables) {
        // fixed Huffman tables: the frame's own transform kernel carries its code words and
        // headers to the device, where they are new there
        bool fresh = false;
        if (const int st1 = fixed_tables(s, fresh)) return st1;
        imp = fresh ? &s : nullptr;
    } else {
        s.fixed.gen = 0;  // (per-image tables will overwrite the slot's table buffers)
    }
    a = fdct_args(s, f.maxval, imp);
    st = stats_args(s);
    st.fixed = (flags & kFlagFixedTables) ? 1u : 0u;
    return kOk;
}

int Encoder::phase1(Slot& s, const FrameDesc& f, const uint8_t qy[64], const uint8_t qc[64], uint32_t flags,
                    Slot* imp, bool export_hist) {
    FdctArgs a;
    StatsArgs st2;
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = lat_prof_ ? clk::now() : clk::time_point{};
    if (const int st = prep1(s, f, qy, qc, flags, imp, a, st2)) return st;
    const clk::time_point t1 = lat_prof_ ? clk::now() : clk::time_point{};
    s.timed = timing_every_ && (frame_counter_++ % (uint64_t)timing_every_) == 0;
    s.count_symbols = s.timed;
    // sampled frames: each kernel launched with its own events (KTimer, kernels.hpp)
    const KTimer t1k{s.ev[0], s.ev[1]}, t2k{s.ev[2], s.ev[3]};
    s.seq = ++seq_counter_;
    s.hist = st2.hist;
    if (export_hist) {  // (by K2's last workgroup: no launch of its own)
        st2.done = reinterpret_cast<uint32_t*>(s.d_ctl + CtlLayout(slot_layout(s).grid()).done + kStatsDoneOff);
        st2.host_cnt = s.d_hist_host->cnt;
        st2.host_key = s.d_hist_host->key;
        st2.host_seq = &s.d_hist_host->seq;
        st2.seq = s.seq;
    }
    JPGE_HIP(launch_fdct(a, s.stream, s.timed ? &t1k : nullptr));
    const clk::time_point t2 = lat_prof_ ? clk::now() : clk::time_point{};
    JPGE_HIP(launch_stats(st2, s.stream, s.timed ? &t2k : nullptr));
    if (export_hist) s.export_queued.store(1, std::memory_order_release);
    if (lat_prof_) {
        lat_ns_[6] += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
        lat_ns_[7] += std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count();
    }
    return kOk;
}

// A frame set's phase 1: the members' arguments come from prep1 (members it refused
// are not in the set).  Their histograms leave through a later code kernel or
// launch_hist_export.
// K1 workgroups per frame of a set (unless JPGE_FDCT_WGS is given): a set's launch has
// n times the tiles, so fewer, longer-lived workgroups per frame (4K, 4 lanes: 214.6 vs
// 212.4 GPix/s with the single-frame cap of 512; alone, a set of 4 in 48 instead of 52 us)
constexpr uint32_t kSetFdctWgs = 256;
int Encoder::phase1_set(Slot* const* s, int n, const FdctArgs* a_in, const StatsArgs* st) {
    FdctArgs a[kMaxSet];
    for (int m = 0; m < n; ++m) {
        a[m] = a_in[m];
        if (!fdct_wgs_ && n > 1) a[m].wgs = kSetFdctWgs;
    }
    // a sampled set: its launches timed with the first member's events, as n frames' work
    // (the other members stay untimed, as Slot::begin left them)
    const uint64_t c = frame_counter_.fetch_add((uint64_t)n);
    Slot& t = *s[0];
    const uint64_t E = (uint64_t)timing_every_;
    t.timed = E && (c + E - 1) / E * E <= c + (uint64_t)n - 1;  // (a sampled frame number in the set)
    t.timed_frames = n;
    for (int m = 0; m < n; ++m) s[m]->count_symbols = t.timed;
    const KTimer t1{t.ev[0], t.ev[1]}, t2{t.ev[2], t.ev[3]};
    JPGE_HIP(launch_fdct_set(a, n, t.stream, t.timed ? &t1 : nullptr));
    JPGE_HIP(launch_stats_set(st, n, t.stream, t.timed ? &t2 : nullptr));
    for (int m = 0; m < n; ++m) {
        s[m]->seq = ++seq_counter_;
        s[m]->hist = st[m].hist;
    }
    return kOk;
}

// Phase 2a (host; the calling thread or a lane's thread): wait for the histograms,
// build the four tables (generateHuffmanCode semantics, Huffman.cpp:3-35) and the
// headers into the slot's pinned staging buffer.
int Encoder::build_tables(Slot& s, bool parallel, TableHelper* helper) {
    // (frames above kFirstSleepMaxPixels nap even on a single lane: their kernels take
    // milliseconds, and a spinning thread would burn a core for them)
    const bool big = (uint64_t)s.g.width * s.g.height > kFirstSleepMaxPixels;
    if (const int w = wait_seq(&s.h_hist->seq, s.seq, s.stream, nap_ || big ? nap_us_ : (parallel ? 0 : hist_nap_us_), &s.export_queued,
                               s.inline_tables ? s.guess_hist : nullptr))
        return w;
    if (lat_prof_) lat_hist_seen_ = std::chrono::steady_clock::now();
    const int64_t t0 = cpu_prof_ ? thread_cpu_ns() : 0;
    // (the tables read the mapped export in place: the keys stay inverted, and only the
    // present symbols' keys are read)
    const int64_t t1 = cpu_prof_ ? thread_cpu_ns() : 0;
    const int r = build_tables_from(s, s.h_hist->cnt, s.h_hist->key, parallel, /*inverted=*/true, helper);
    if (cpu_prof_) {
        cpu_read_ns_.fetch_add(t1 - t0, std::memory_order_relaxed);
        cpu_build_ns_.fetch_add(thread_cpu_ns() - t1, std::memory_order_relaxed);
        cpu_builds_.fetch_add(1, std::memory_order_relaxed);
    }
    return r;
}

// The four tables from counts and first-occurrence keys, and the headers (the
// image's real dimensions in SOF0), into the slot's pinned staging buffer.
int Encoder::build_tables_from(Slot& s, const uint32_t* cnt_all, const uint64_t* first_all, bool parallel,
                               bool inverted, TableHelper* helper) {
    const int64_t t0 = cpu_prof_ ? thread_cpu_ns() : 0;
    s.fixed.gen = 0;  // (the slot's table buffers get this frame's own tables)
    HuffTable tabs[4];
    int ok[4] = {0, 0, 0, 0};
    // the four tables are independent; the AC tables dominate
    auto one = [&](long t) {
        ok[t] = inverted ? build_table_inverted(cnt_all + t * 256, first_all + t * 256, tabs[t])
                         : build_table(cnt_all + t * 256, first_all + t * 256, tabs[t]);
    };
    const bool gray = s.g.gray();
    if (gray) {
        // one component: the two luma tables; the chroma texts are empty and never reach the
        // builder, and their slots of the table block stay unused (zeroed)
        parallel_for(2, parallel ? 2 : 1, one);
        ok[2] = ok[3] = 1;
        std::memset(s.h_tab + 2 * 256, 0, 2 * 256 * sizeof(uint32_t));
    } else if (helper && helper->post(cnt_all, first_all, inverted, tabs, ok)) {
        one(1);  // (the luma AC table here, the other three on the helper)
        helper->wait();
    } else {
        parallel_for(4, parallel ? 4 : 1, one);
    }
    const int64_t t1 = cpu_prof_ ? thread_cpu_ns() : 0;
    for (int t = 0; t < (gray ? 2 : 4); ++t)
        if (ok[t])
            for (int i = 0; i < 256; ++i)
                s.h_tab[t * 256 + i] = ((uint32_t)tabs[t].len[i] << 16) | (tabs[t].code[i] & 0xFFFF);
    const int64_t t2 = cpu_prof_ ? thread_cpu_ns() : 0;
    const int bad = !(ok[0] & ok[1] & ok[2] & ok[3]);
    uint64_t nsym = 0;
    for (int i = 0; i < 1024; ++i) nsym += cnt_all[i];
    s.symbols = nsym;
    if (bad) {
        if (std::getenv("JPGE_DEBUG")) {
            std::fprintf(stderr, "jpge: table build failed (seq %llu):", (unsigned long long)s.seq);
            for (int t = 0; t < 4; ++t) {
                uint64_t n = 0;
                for (int i = 0; i < 256; ++i) n += cnt_all[t * 256 + i];
                std::fprintf(stderr, " t%d ok=%d n=%llu", t, ok[t], (unsigned long long)n);
            }
            std::fprintf(stderr, "\n");
        }
        return kErrInternal;
    }
    const HuffTable* tp[4] = {&tabs[0], &tabs[1], &tabs[2], &tabs[3]};
    const std::vector<uint8_t> hdr = gray ? jfif_headers_gray(s.img_w, s.img_h, s.qy, tp, restart_mcus_)
                                          : jfif_headers(s.img_w, s.img_h, s.qy, s.qc, tp, restart_mcus_,
                                                         (uint8_t)((s.g.yh << 4) | s.g.yv()));
    if (hdr.size() > kHdrMax) return kErrInternal;
    std::memcpy(reinterpret_cast<uint8_t*>(s.h_tab) + kTabBytes, hdr.data(), hdr.size());
    s.hdr_len = hdr.size();
    if (cpu_prof_) {
        cpu_part_ns_[0].fetch_add(t1 - t0, std::memory_order_relaxed);
        cpu_part_ns_[1].fetch_add(t2 - t1, std::memory_order_relaxed);
        cpu_part_ns_[2].fetch_add(thread_cpu_ns() - t2, std::memory_order_relaxed);
    }
    if (s.out_cap && s.out_cap < s.hdr_len + 2) return kErrNoSpace;
    return kOk;
}

// Tables + headers to the device by a copy (when no transform kernel carries them).
int Encoder::import_tables_copy(Slot& s) {
    JPGE_HIP(hipMemcpyAsync(s.d_tab, s.h_tab, kTabBytes + s.hdr_len, hipMemcpyHostToDevice, s.stream));
    return kOk;
}

int Encoder::export_hist(Slot& s) {
    JPGE_HIP(launch_hist_export(s.hist, s.d_hist_host->cnt, s.d_hist_host->key, &s.d_hist_host->seq, s.seq, s.stream));
    s.export_queued.store(1, std::memory_order_release);
    return kOk;
}

// Phase 2b (GPU): the entropy kernels (tables already on the device); `exp`: a
// later frame whose histograms the code kernel exports on the way.
int Encoder::launch_entropy_phase(Slot& s, Slot* exp, bool lone, int parts) {
    EntropyArgs e = entropy_args(s);
    // A single image on a 1-lane encoder (encode()): the result is handed over once every
    // pack workgroup's write-through stores have completed, so the call need not wait for
    // the kernel's formal end (9 us per 4K call).  The pipeline streams its stores
    // instead (write-through cost it 1.3%) and awaits its stream at the batch's end.
    if (lone && lanes_.size() == 1)
        e.pack_done = reinterpret_cast<uint32_t*>(s.d_ctl + CtlLayout(slot_layout(s).grid()).done + kPackDoneOff);
    if (parts == 3) s.h_result[2] = 0;  // (the slot's previous entropy kernel finished before phase1; gated: encode())
    Slot::carry_export(e, exp);
    const KTimer tc{s.ev[4], s.ev[5]}, tp{s.ev[6], s.ev[7]};
    if (parts & 1) JPGE_HIP(launch_entropy_code(e, s.stream, s.timed ? &tc : nullptr));
    if (parts & 2) JPGE_HIP(launch_entropy_pack(e, s.stream, s.timed ? &tp : nullptr));
    return kOk;
}

int Encoder::finish(Slot& s, FrameDesc& f, uint32_t flags, bool guess_wait, const std::function<bool()>* idle) {
    // (a first sleep only up to kFirstSleepMaxPixels: 16384^2 frames, few per lane and
    // irregular, lost 3.7% to it)
    // (a set's later members: their results follow the first one's within microseconds,
    // and their short waits would blur the estimate of the real one)
    WaitGuess* const guess =
        guess_wait && (uint64_t)s.g.width * s.g.height <= kFirstSleepMaxPixels ? s.guess_result : nullptr;
    const bool big = (uint64_t)s.g.width * s.g.height > kFirstSleepMaxPixels;  // (as build_tables)
    if (const int w = wait_seq(&s.h_result[3], s.seq, s.stream, nap_ || big ? nap_us_ : 0, nullptr, guess, idle)) return w;
    if (s.timed) {
        JPGE_HIP(wait_event(s.ev[7]));
        std::lock_guard<std::mutex> g(times_mu_);
        float code = 0, pack = 0;
        hipEventElapsedTime(&times_.fdct, s.ev[0], s.ev[1]);
        hipEventElapsedTime(&times_.dc_stats, s.ev[2], s.ev[3]);
        hipEventElapsedTime(&code, s.ev[4], s.ev[5]);
        hipEventElapsedTime(&pack, s.ev[6], s.ev[7]);
        hipEventElapsedTime(&times_.entropy, s.ev[4], s.ev[7]);
        hipEventElapsedTime(&times_.total, s.ev[0], s.ev[7]);
        times_.fdct_sum += times_.fdct;
        times_.dc_stats_sum += times_.dc_stats;
        times_.entropy_sum += times_.entropy;
        times_.code_sum += code;
        times_.pack_sum += pack;
        times_.frames += s.timed_frames;                       // (the launches' frames)
        times_.launches += 1;
    }
    if (s.count_symbols) {  // (every member of a timed set: the launches' record bytes are the sum over them)
        std::lock_guard<std::mutex> g(times_mu_);
        times_.symbols += s.symbols;
    }
    if (stamps_file_) hipStreamSynchronize(s.stream);
    dump_stamps(s);
    const uint64_t err = s.h_result[1] | s.h_result[2];
    if (err & 4) { f.len = 0; return kErrNoSpace; }
    if (err) return kErrTimeout;
    const size_t len = (size_t)s.h_result[0];
    f.len = len;
    if (flags & kFlagDeviceOutput) return kOk;
    if (len > f.cap) return kErrNoSpace;
    // Queued on the lane's stream and not awaited here: every caller synchronises the
    // stream afterwards (a batch at its end), and the slot's next pack kernel is behind
    // the copy in stream order.  (Waiting here held the lane's host thread for the
    // stream's queued kernels too: 77 GPix/s with host outputs.)
    JPGE_HIP(hipMemcpyAsync(f.out, s.out_dev, len, hipMemcpyDeviceToHost, s.stream));
    return kOk;
}

int Encoder::encode(FrameDesc& f, const uint8_t qy[64], const uint8_t qc[64], uint32_t flags) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    flags &= ~kFlagFixedTables;
    if (huff_mode_) return encode_fixed(f, qy, qc, flags | kFlagFixedTables);
    Slot& s = slot0();
    using clk = std::chrono::steady_clock;
    clk::time_point T[6];
    if (lat_prof_) T[0] = clk::now();
    int st = phase1(s, f, qy, qc, flags, nullptr, true);
    // The gate: the tables' copy and the code kernel are queued now, behind a stream wait
    // on a mapped word the host sets once the tables are in h_tab, so their launches
    // overlap K1 and K2 instead of following the tables (the pack kernel's arguments
    // carry the header length, so it is launched after them, while the code kernel
    // runs).  Every path below opens the gate.  (A failed table build: the code kernel
    // reads the tables h_tab holds, valid ones or zeros, and its output is discarded.)
    struct Gate {  // (opened at the latest when the call unwinds)
        uint32_t* word;
        uint32_t value;  // (the word holds the previous gated call's value, one less)
        bool shut = false;
        void open() {
            if (shut) __atomic_store_n(word, value, __ATOMIC_RELEASE);
            shut = false;
        }
        ~Gate() { open(); }
    } gate{s.gate(), gate_count_ + 1};
    if (!st && gate_) ++gate_count_;
    if (!st && gate_ == 1) {  // a workgroup of ours waits and copies (entropy.hip gate_copy_kernel)
        s.h_result[2] = 0;  // (its time-out flag)
        if (launch_gate_copy(reinterpret_cast<const uint32_t*>(s.d_result_host + 6), gate.value, s.d_tab_host, s.d_tab,
                             (uint32_t)((kTabBytes + kHdrMax) / 16), s.d_result_host + 2, gate_ticks_,
                             s.stream) == hipSuccess) {
            gate.shut = true;
            st = launch_entropy_phase(s, nullptr, /*lone=*/true, /*parts=*/1);
            if (st) gate.open();
        } else {
            st = kErrHip;
        }
    } else if (!st && gate_ == 2) {  // the runtime's stream wait, then a copy
        if (hipStreamWaitValue32(s.stream, gate.word, gate.value, hipStreamWaitValueEq, 0xFFFFFFFFu) == hipSuccess) {
            gate.shut = true;
            s.h_result[2] = 0;
            if (hipMemcpyAsync(s.d_tab, s.h_tab, kTabBytes + kHdrMax, hipMemcpyHostToDevice, s.stream) != hipSuccess)
                st = kErrHip;
            if (!st) st = launch_entropy_phase(s, nullptr, /*lone=*/true, /*parts=*/1);
            if (st) gate.open();
        } else {
            (void)hipGetLastError();
        }
    }
    if (lat_prof_) T[1] = clk::now();
    // The tables: on this thread, with the helper thread of a 1-lane encoder for frames
    // of 1 MPix and up (armed now, so its wake-up overlaps the kernels; spawning threads
    // per call would cost more than the tables it overlaps).  Not above
    // kFirstSleepMaxPixels: the helper spins from here to the histograms, which take
    // milliseconds there, for tables that are a small part of such a call.
    TableHelper* helper = nullptr;
    uint32_t cw, ch;  // (the coded frame's pixels)
    coded_size(f.width, f.height, plan_settings(), &cw, &ch);
    const uint64_t npx = (uint64_t)cw * ch;
    if (!st && table_helper_ && lanes_.size() == 1 && npx >= (1u << 20) && npx <= kFirstSleepMaxPixels) {
        if (!helper_) helper_.reset(new TableHelper());
        helper = helper_.get();
        helper->arm();
    }
    if (!st) st = build_tables(s, false, helper);
    if (helper) helper->disarm();
    if (lat_prof_) T[2] = clk::now();
    const bool gated = gate.shut;
    if (gate.shut) {
        if (gate_delay_us_) std::this_thread::sleep_for(std::chrono::microseconds(gate_delay_us_));  // (tests)
        gate.open();
        if (!st) st = launch_entropy_phase(s, nullptr, /*lone=*/true, /*parts=*/2);
    } else {
        if (!st) st = import_tables_copy(s);
        if (!st) st = launch_entropy_phase(s, nullptr, /*lone=*/true);
    }
    if (lat_prof_) T[3] = clk::now();
    if (!st) st = finish(s, f, flags);
    if (st == kErrTimeout && gated && s.h_result[2] == 1) {
        // The gate kernel timed out before the host opened it (a host thread stalled for
        // longer than the time-out): the code kernel ran on stale tables, so the frame is
        // coded again behind a plain copy of the tables now in h_tab.
        gate_timeouts_.fetch_add(1, std::memory_order_relaxed);
        s.h_result[2] = 0;
        s.seq = ++seq_counter_;
        st = import_tables_copy(s);
        if (!st) st = launch_entropy_phase(s, nullptr, /*lone=*/true);
        if (!st) st = finish(s, f, flags);
    }
    if (lat_prof_) T[4] = clk::now();
    st = await_call_end(s, flags, st);
    if (lat_prof_ && !st) {
        T[5] = clk::now();
        auto ns = [](clk::time_point a, clk::time_point b) {
            return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count();
        };
        lat_ns_[0] += ns(T[0], T[1]);
        lat_ns_[1] += ns(T[1], lat_hist_seen_);
        lat_ns_[2] += ns(lat_hist_seen_, T[2]);
        lat_ns_[3] += ns(T[2], T[3]);
        lat_ns_[4] += ns(T[3], T[4]);
        lat_ns_[5] += ns(T[4], T[5]);
        ++lat_calls_;
    }
    f.status = st;
    return st;
}

// A single image with fixed Huffman tables: the tables and the headers are known before
// the frame, so the four kernels are queued back to back (K1 carrying the code words and
// headers to the device where the slot does not hold them yet), and the call waits for the
// pack kernel's result word alone: no gate kernel, no table thread, no histogram wait.
int Encoder::encode_fixed(FrameDesc& f, const uint8_t qy[64], const uint8_t qc[64], uint32_t flags) {
    Slot& s = slot0();
    int st = phase1(s, f, qy, qc, flags, nullptr, /*export_hist=*/false);
    if (!st) st = launch_entropy_phase(s, nullptr, /*lone=*/true);
    if (st) s.fixed.gen = 0;  // (the tables may not have reached the device)
    if (!st) st = finish(s, f, flags);
    st = await_call_end(s, flags, st);
    f.status = st;
    return st;
}

// Every output byte of a single image is in place.  Device output on a 1-lane encoder: the
// result word is written once every pack workgroup's (write-through) stores have
// completed, so the kernel's formal end is not awaited (the stream orders the context's
// next work after it; ~9 us).  Host output: the copy queued by finish(), awaited by
// spinning as a batch lane's end (a blocking stream synchronisation adds tens of us of
// wake-up).
int Encoder::await_call_end(Slot& s, uint32_t flags, int st) {
    if (!st && (flags & kFlagDeviceOutput) && lanes_.size() == 1) return st;
    if (hipEventRecord(lanes_[0]->done, s.stream) != hipSuccess)
        hipStreamSynchronize(s.stream);
    else if (wait_event(lanes_[0]->done) != hipSuccess && !st)
        st = kErrHip;
    return st;
}

int Encoder::encode_batch(FrameDesc* fr, int n, const uint8_t qy[64], const uint8_t qc[64], uint32_t flags) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    const auto t_enter = std::chrono::steady_clock::now();
    JPGE_HIP(hipSetDevice(device_));
    for (int i = 0; i < n; ++i) fr[i].status = 0;
    if (n <= 0) return kOk;
    // (fixed Huffman tables: the lanes run the pipeline without the host in the middle)
    flags = (flags & ~kFlagFixedTables) | (huff_mode_ ? kFlagFixedTables : 0u);
    // Frames are dealt dynamically: a lane takes the batch's next frame (or frame set)
    // when its pipeline has room, so lanes finish together.  Lane 0 runs on the calling
    // thread.
    const int set = batch_set_size(fr, n);
    const int nl = std::min<int>((int)lanes_.size(), (n + set - 1) / set);
    for (int l = 0; l < nl; ++l)
        if (const int st = add_slots(*lanes_[l], (lookahead_ + drain_lag_ + 1) * set)) return st;
    std::atomic<int> next{0};
    for (int l = 1; l < nl; ++l)
        lanes_[l]->post([this, l, fr, n, &next, set, qy, qc, flags] {
            hipSetDevice(device_);
            return run_lane(*lanes_[l], fr, n, &next, set, qy, qc, flags);
        });
    // (napping on the calling thread: ~1 us timer slack for the call, restored after)
    const long slack = nap_ ? prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0) : -1;
    if (slack > 0) prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    int st = run_lane(*lanes_[0], fr, n, &next, set, qy, qc, flags);
    if (slack > 0) prctl(PR_SET_TIMERSLACK, (unsigned long)slack, 0, 0, 0);
    const auto t_lane0 = std::chrono::steady_clock::now();
    for (int l = 1; l < nl; ++l) {
        const int e = lanes_[l]->wait();
        if (!st) st = e;
    }
    if (host_trace_file_) {
        std::lock_guard<std::mutex> g(trace_mu_);
        if (FILE* f = std::fopen(host_trace_file_, "a")) {
            std::fprintf(f, "-2 -2 0 -1 %.2f %.2f %.2f\n", abs_us(t_enter), abs_us(t_lane0),
                         abs_us(std::chrono::steady_clock::now()));
            std::fclose(f);
        }
    }
    int bad = st;
    for (int i = 0; i < n && !bad; ++i) bad = fr[i].status;
    if (bad)  // an error exit (run_lane's early returns included) may leave device-to-host
              // copies into the caller's buffers queued: drain every lane before returning
        for (int l = 0; l < nl; ++l) hipStreamSynchronize(lanes_[l]->stream);
    for (int i = 0; i < n; ++i)  // the first failing frame's status
        if (fr[i].status) return fr[i].status;
    return st;
}

// Frames per launch: sets of frames of one geometry (kernels.hpp FrameSet), up to
// kMaxSet and about four 4K frames' pixels per launch (4K: 192 -> 208 GPix/s with sets
// of 4, 203 with 2; 1080p batch: 111 -> 143).  A set's entropy launch needs every member
// placed by its own last code workgroup (the pipeline's placement mode, no restart
// intervals).
constexpr uint64_t kSetPixels = 4ull * 3840ull * 2160ull;
int Encoder::batch_set_size(const FrameDesc* fr, int n) const {
    if (n < 2 || set_ == 1) return 1;
    const FrameDesc& f0 = fr[0];
    if (!f0.width || !f0.height || f0.width > 65535 || f0.height > 65535) return 1;
    for (int i = 1; i < n; ++i)
        if (fr[i].width != f0.width || fr[i].height != f0.height || (fr[i].maxval == 255) != (f0.maxval == 255) ||
            fr[i].fmt != f0.fmt)
            return 1;
    const bool placed_in_code = (ext_place_ > 0 || (ext_place_ < 0 && lanes_.size() > 1)) && place_in_code_;
    // (downscaled frames: one source size and one factor give one output geometry, which is
    // the one the kernels after K1 and the set's size go by)
    // (oriented frames: the oriented frame's, likewise; plan_frame refuses both settings together)
    uint32_t w0, h0;
    coded_size(f0.width, f0.height, plan_settings(), &w0, &h0);
    const Geometry g0 = fmt_gray(f0.fmt) ? gray_geometry(w0, h0) : geometry(w0, h0, mode_);
    if (!placed_in_code || restart_mcus_ || layout(g0).grid() > kPlaceInCodeMaxWgs) return 1;
    if (set_) return set_;
    const uint64_t k = kSetPixels / ((uint64_t)w0 * h0);
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(kMaxSet, k));
}

// A lane's state for one batch, and the pipeline's steps over it; run_lane puts the steps
// in their order.  Pipeline step t handles frame set t of this lane: frames mine[t*set ..],
// each in slot (t mod S) * set + member.  Only the lane's last set may be short.  Arrays of
// a set's slots are indexed by member; a null entry is a member that is not taking part.
struct Encoder::LaneRun {
    Encoder& enc;
    Lane& ln;
    FrameDesc* const frames;
    const int total;
    std::atomic<int>* const next;
    const int set;
    const uint8_t* const qy;
    const uint8_t* const qc;
    const uint32_t flags;
    const bool fixed;       // fixed Huffman tables (kFlagFixedTables)
    const int S;            // slot sets (add_slots: >= lookahead + drain lag + 1)
    std::vector<int> mine;  // batch indices of the frames this lane took, in its order
    // Per-image tables: this lane's frames whose tables are not built yet.  The lane's waits
    // build any whose histograms are in (the ~25 us of a 1080p frame's tables fill a wait
    // instead of a worker's polling and hand-off), and a frame's entropy launch builds its
    // own if they are still missing.
    std::vector<Slot*> pend;
    int n = 0;         // sets taken so far
    bool open = true;  // the batch may still have frames
    int first_err = kOk;

    LaneRun(Encoder& e, Lane& l, FrameDesc* fr, int tot, std::atomic<int>* nx, int st, const uint8_t* y,
            const uint8_t* c, uint32_t fl)
        : enc(e), ln(l), frames(fr), total(tot), next(nx), set(st), qy(y), qc(c), flags(fl),
          fixed((fl & kFlagFixedTables) != 0), S((int)l.slots.size() / st) {
        mine.reserve(total);
    }
    int members(int t) const { return std::min(set, (int)mine.size() - t * set); }
    FrameDesc& frame(int t, int m) const { return frames[mine[t * set + m]]; }
    Slot& slot(int t, int m) const { return *ln.slots[(t % S) * set + m]; }
    void note(int t, int m, int st) {
        if (st && fixed) slot(t, m).fixed.gen = 0;  // (its tables may not have reached the device)
        if (st && !frame(t, m).status) frame(t, m).status = st;
        if (st && !first_err) first_err = st;
    }
    // Step i has room for a new set: take the batch's next frames.
    void take(int i) {
        if (!open || i != n) return;
        const int g = next->fetch_add(set, std::memory_order_relaxed);
        if (g < total) {
            for (int m = 0; m < set && g + m < total; ++m) mine.push_back(g + m);
            ++n;
        } else {
            open = false;
        }
    }

    // Queue K1 and K2 of set i into out[].  imp[m]: the slot whose tables and headers member
    // m's K1 carries to the device (fixed tables: none).  lone_exports: a single frame's K2
    // exports its own histograms when it has no partner (whose code kernel would).  A
    // single frame takes the 1-member kernel instances, a set one launch per kernel.
    void queue_phase1(int i, Slot* const* imp, bool lone_exports, Slot** out) {
        if (set == 1) {
            Slot& s = slot(i, 0);
            note(i, 0, enc.phase1(s, frame(i, 0), qy, qc, flags, imp[0], lone_exports && !imp[0]));
            if (!frame(i, 0).status) out[0] = &s;
            return;
        }
        Slot* ss[kMaxSet];
        FdctArgs fa[kMaxSet];
        StatsArgs sa[kMaxSet];
        int ms[kMaxSet], ok = 0;
        for (int m = 0; m < members(i); ++m) {
            Slot& s = slot(i, m);
            const int st = enc.prep1(s, frame(i, m), qy, qc, flags, imp[m], fa[ok], sa[ok]);
            note(i, m, st);
            if (st) continue;
            ss[ok] = &s;
            ms[ok++] = m;
        }
        if (!ok) return;
        const int st = enc.phase1_set(ss, ok, fa, sa);
        for (int q = 0; q < ok; ++q) {
            note(i, ms[q], st);
            if (!st) out[ms[q]] = ss[q];
        }
    }

    // Queue the entropy kernels of set t's members in s[] (tables on the device or on their
    // way): one launch per kernel for the set, or frame by frame (a single frame; a member
    // its code kernel does not place).  carry (or null): member m's code kernel exports
    // carry[m]'s histograms on the way, which is noted there.  A member whose launch failed
    // leaves s[].
    void queue_entropy(int t, Slot** s, Slot* const* carry) {
        EntropyArgs ea[kMaxSet];
        int ms[kMaxSet], ne = 0;
        bool as_set = set > 1;
        Slot* tm = nullptr;  // (a sampled set's member: its events time the launches)
        for (int m = 0; m < members(t); ++m) {
            if (!s[m]) continue;
            ea[ne] = enc.entropy_args(*s[m]);
            if (carry && carry[m]) Slot::carry_export(ea[ne], carry[m]);
            as_set = as_set && ea[ne].done;
            if (s[m]->timed && !tm) tm = s[m];
            ms[ne++] = m;
        }
        if (!ne) return;
        if (as_set) {
            for (int q = 0; q < ne; ++q) s[ms[q]]->h_result[2] = 0;
            const KTimer tc{tm ? tm->ev[4] : nullptr, tm ? tm->ev[5] : nullptr};
            const KTimer tp{tm ? tm->ev[6] : nullptr, tm ? tm->ev[7] : nullptr};
            const hipError_t e = launch_entropy_set(ea, ne, s[ms[0]]->stream, tm ? &tc : nullptr, tm ? &tp : nullptr);
            for (int q = 0; q < ne; ++q) {
                note(t, ms[q], e == hipSuccess ? kOk : kErrHip);
                if (e != hipSuccess) s[ms[q]] = nullptr;
            }
        } else {
            for (int q = 0; q < ne; ++q) {
                const int m = ms[q];
                const int st = enc.launch_entropy_phase(*s[m], carry ? carry[m] : nullptr);
                note(t, m, st);
                if (st) s[m] = nullptr;
            }
        }
        for (int q = 0; carry && q < ne; ++q)
            if (s[ms[q]] && carry[ms[q]]) carry[ms[q]]->export_queued.store(1, std::memory_order_release);
    }

    // Drain set k: its results, and its host outputs' copies queued.  idle: work for the
    // waits while frames' tables are pending.
    void drain(int k, const std::function<bool()>* idle) {
        for (int m = 0; m < members(k); ++m) {
            Slot& s = slot(k, m);
            if (!frame(k, m).status)
                note(k, m, enc.finish(s, frame(k, m), flags, /*guess_wait=*/m == 0, pend.empty() ? nullptr : idle));
            else hipStreamSynchronize(s.stream);
        }
    }
};

// One software pipeline on the lane's stream (steps are lane-local), in two stage
// schedules over LaneRun's steps.
//
// Per-image tables.  Step i queues
//   K1(i) [carrying set j = i-L's tables + headers to the device], K2(i),
//   then set j's entropy kernels [the code kernel carrying set i's histograms to
//   the host for a table worker],
// so the host builds a set's tables while the GPU works through the L sets queued
// ahead of its entropy launch; set i-L-D is drained D steps after that launch (about
// D sets of queued GPU work while the host waits).  Member m of one set pairs with
// member m of the other for the carried duties.  The pipeline's edges fall back to a
// standalone export kernel and a table copy.
//
// Fixed tables: the same with L = 0 and nothing carried.  Nothing of a frame waits on the
// host: its tables and headers are known when it is queued (fixed_tables), so step i queues
// K1(i), K2(i) (the instance without histograms) and set i's entropy kernels back to back,
// and drains set i-D.  There is no histogram export, no table import of another set and no
// table build.
int Encoder::run_lane(Lane& ln, FrameDesc* frames, int total, std::atomic<int>* next, int set, const uint8_t qy[64],
                      const uint8_t qc[64], uint32_t flags) {
    LaneRun r(*this, ln, frames, total, next, set, qy, qc, flags);
    const bool fixed = r.fixed;
    const int L = fixed ? 0 : lookahead_, D = drain_lag_;
    if (!fixed) r.pend.reserve((size_t)(L + D + 2) * set);
    std::vector<Slot*>& pend = r.pend;
    const std::function<bool()> build_ready = [&]() -> bool {
        for (size_t q = 0; q < pend.size(); ++q) {
            Slot& s = *pend[q];
            if (s.tables_done.load(std::memory_order_relaxed)) {
                pend.erase(pend.begin() + (long)q);
                return true;
            }
            if (__atomic_load_n(&s.h_hist->seq, __ATOMIC_ACQUIRE) != s.seq) continue;
            pend.erase(pend.begin() + (long)q);
            s.tables_status = build_tables(s, false);
            s.tables_done.store(1, std::memory_order_release);
            return true;
        }
        return false;
    };
    auto submit_tables = [&](Slot& s) {
        s.tables_done.store(0, std::memory_order_relaxed);
        s.inline_tables = true;
        pend.push_back(&s);
    };
    // diagnostic host trace: (step, point, us since the call, and at point 1 the
    // awaited table job's submit / start / done times)
    std::vector<std::array<double, 6>> trace;
    const auto t_call = std::chrono::steady_clock::now();
    auto us = [&](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::micro>(t - t_call).count();
    };
    // diagnostic (JPGE_CPU_PROF): this thread's CPU time per loop segment, summed per encoder
    int64_t cpu_last = cpu_prof_ ? thread_cpu_ns() : 0;
    int64_t cpu_acc[6] = {0, 0, 0, 0, 0, 0};
    auto mark = [&](int i, int point, const Slot* job = nullptr) {
        if (cpu_prof_) {
            const int64_t t = thread_cpu_ns();
            cpu_acc[point] += t - cpu_last;
            cpu_last = t;
        }
        if (host_trace_file_)
            trace.push_back({(double)i, (double)point, us(std::chrono::steady_clock::now()),
                             job ? us(job->t_submit) : 0.0, job ? us(job->t_start) : 0.0,
                             job ? us(job->t_done) : 0.0});
    };
    for (int i = 0;; ++i) {
        r.take(i);
        if (!r.open && i >= r.n + L + D) break;
        const int j = i - L, k = j - D;
        const bool have_j = j >= 0 && j < r.n;
        mark(i, 0);
        Slot* sj[kMaxSet] = {};  // per-image tables: set j's members, tables built, ready for their entropy kernels
        Slot* si[kMaxSet] = {};  // set i's members, K1 and K2 queued
        for (int m = 0; !fixed && have_j && m < r.members(j); ++m) {
            if (r.frame(j, m).status) continue;
            Slot& s = r.slot(j, m);
            if (!s.tables_done.load(std::memory_order_acquire)) {
                s.tables_status = build_tables(s, /*parallel=*/false);
                s.tables_done.store(1, std::memory_order_release);
            }
            if (s.tables_status) r.note(j, m, s.tables_status);
            else sj[m] = &s;
        }
        mark(i, 1, sj[0]);
        if (i < r.n) r.queue_phase1(i, sj, /*lone_exports=*/!fixed, si);
        for (int m = 0; !fixed && m < kMaxSet; ++m) {
            if (!si[m]) continue;
            // (no code kernel of set j to carry the export, and no K2 of its own did)
            if (!sj[m] && !si[m]->export_queued.load(std::memory_order_relaxed)) r.note(i, m, export_hist(*si[m]));
            if (!r.frame(i, m).status) submit_tables(*si[m]);
        }
        mark(i, 2);
        if (have_j && fixed) {
            r.queue_entropy(i, si, nullptr);  // (j == i)
        } else if (have_j) {
            for (int m = 0; m < kMaxSet; ++m) {  // (the tables K1(i) does not carry: by a copy)
                if (!sj[m] || si[m]) continue;
                const int st = import_tables_copy(*sj[m]);
                r.note(j, m, st);
                if (st) sj[m] = nullptr;
            }
            r.queue_entropy(j, sj, si);
        }
        mark(i, 3);
        for (int m = 0; !fixed && m < kMaxSet; ++m)  // (no carrier after all: set i's histograms on their own)
            if (si[m] && !r.frame(i, m).status && !si[m]->export_queued.load(std::memory_order_relaxed))
                r.note(i, m, export_hist(*si[m]));
        if (k >= 0 && k < r.n) r.drain(k, &build_ready);
        mark(i, 4);
    }
    // every output byte is in place: the stream's tail, awaited by spinning (a
    // blocking stream synchronisation adds tens of us of wake-up latency)
    JPGE_HIP(hipEventRecord(ln.done, ln.stream));
    JPGE_HIP(wait_event(ln.done));
    mark(r.n + L + D, 5);  // (n: this lane's set count)
    if (cpu_prof_) {
        for (int q = 0; q < 6; ++q) cpu_ns_[q].fetch_add(cpu_acc[q], std::memory_order_relaxed);
        cpu_frames_.fetch_add((int64_t)r.mine.size(), std::memory_order_relaxed);
    }
    if (host_trace_file_) {
        std::lock_guard<std::mutex> g(trace_mu_);
        if (FILE* f = std::fopen(host_trace_file_, "a")) {
            for (const auto& t : trace)
                std::fprintf(f, "%d %d %.2f %d %.2f %.2f %.2f\n", (int)t[0], (int)t[1], t[2], ln.id, t[3], t[4], t[5]);
            std::fprintf(f, "-1 -1 0 %d %.2f %.2f 0\n", ln.id, abs_us(t_call),
                         abs_us(std::chrono::steady_clock::now()));
            std::fclose(f);
        }
    }
    return r.first_err;
}

int Encoder::fdct_quant(const FrameDesc& f, const uint8_t qy[64], const uint8_t qc[64], uint32_t flags,
                        int16_t* y, int16_t* cb, int16_t* cr) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    Slot& s = slot0();
    flags &= ~kFlagFixedTables;  // (the stage entries are the same in every Huffman mode)
    int st = phase1(s, f, qy, qc, flags | kFlagDeviceOutput | kFlagCoefficients, nullptr, true);
    if (st) { hipStreamSynchronize(s.stream); return st; }
    JPGE_HIP(hipStreamSynchronize(s.stream));
    const Geometry& g = s.g;
    std::vector<int16_t> coef((size_t)g.nblocks() * 64);
    JPGE_HIP(hipMemcpyAsync(coef.data(), s.d_coef, coef.size() * 2, hipMemcpyDeviceToHost, s.stream));  // (not the null stream)
    JPGE_HIP(hipStreamSynchronize(s.stream));
    const uint32_t ybw = g.yh * g.mw, cbw = g.mw;
    for (uint32_t m = 0; m < g.nmcu(); ++m) {
        const uint32_t mr = m / g.mw, mc = m % g.mw;
        for (int k = 0; k < (int)g.bpm; ++k) {
            const int16_t* src = &coef[((size_t)m * g.bpm + k) * 64];
            const int comp = block_comp(k, g.bpm);
            int16_t* dst;
            if (comp == 0) dst = y + ((size_t)(mr * g.yv() + k / g.yh) * ybw + mc * g.yh + k % g.yh) * 64;
            else dst = (comp == 1 ? cb : cr) + ((size_t)mr * cbw + mc) * 64;
            for (int i = 0; i < 64; ++i) dst[i] = src[i];
        }
    }
    return kOk;
}

int Encoder::symbol_stats(const FrameDesc& f, const uint8_t qy[64], const uint8_t qc[64], uint32_t flags,
                          uint32_t counts[1024], uint64_t first[1024]) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    Slot& s = slot0();
    flags &= ~kFlagFixedTables;
    int st = phase1(s, f, qy, qc, flags | kFlagDeviceOutput, nullptr, true);
    if (st) { hipStreamSynchronize(s.stream); return st; }
    JPGE_HIP(hipStreamSynchronize(s.stream));
    read_hist(*s.h_hist, counts, first);
    return kOk;
}

Encoder::Slot& Encoder::slot0() { return *lanes_[0]->slots[0]; }

}  // namespace jpge
