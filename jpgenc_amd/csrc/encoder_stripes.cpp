// Row stripes of a larger image (one stripe per device): the Encoder's
// stripe phases.
#include "encoder_impl.hpp"

#include <algorithm>

namespace jpge {

// A stripe is the MCU rows [mcu_row0, mcu_row0 + mcu_rows) of a width x height
// image; its own geometry has the stripe's real pixel rows (the last stripe's bottom
// padding replicates the image's last row, Image.cpp:511-519).  Every phase runs on
// lane 0's first slot and returns when its results are on the host.
int Encoder::stripe_transform(const StripeDesc& d, const uint8_t qy[64], const uint8_t qc[64], int32_t last_dc[3]) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    if (!stripe_settings_ok(fmt_, plan_settings(), huff_mode_ != 0)) return kErrArg;
    if (!d.rgb || !last_dc || d.width == 0 || d.height == 0 || d.width > 65535 || d.height > 65535) return kErrArg;
    if (d.maxval < 1 || d.maxval > 255) return kErrRange;
    const uint32_t mh_img = (d.height + 15) / 16;
    if (d.mcu_rows == 0 || d.mcu_row0 >= mh_img || d.mcu_rows > mh_img - d.mcu_row0) return kErrArg;
    const size_t row = (size_t)fmt_row_bytes(fmt_, d.width), stride = d.stride ? d.stride : row;
    if (stride < row) return kErrArg;
    if (!tables_nonzero(qy, qc)) return kErrArg;
    const uint32_t hs = std::min(16 * d.mcu_rows, d.height - 16 * d.mcu_row0);
    const Geometry g = geometry(d.width, hs);
    if (!k1_offsets_fit(fmt_, g, stride)) return kErrArg;  // (the kernel's 32-bit offsets span the stripe)
    // restart intervals: the stripe must start one (its bytes are then its own)
    if (restart_mcus_ && ((uint64_t)d.mcu_row0 * g.mw) % restart_mcus_ != 0) return kErrArg;
    Slot& s = slot0();
    if (const int st = ensure(s, g, 0, 0)) return st;
    // (no output yet: stripe_code sizes the headers without one, stripe_pack takes the caller's)
    FrameInput in;
    in.ptr = d.rgb;
    in.stride = stride;
    in.fmt = fmt_;
    s.begin(g, qy, qc, in, nullptr, 0, restart_mcus_, d.width, d.height);
    s.rst.mcu0 = d.mcu_row0 * g.mw;
    s.key_y0 = 2ull * d.mcu_row0 * (2ull * g.mw);  // Y blocks above the stripe (raster)
    s.key_c0 = (uint64_t)d.mcu_row0 * g.mw;         // Cb blocks above it
    s.key_ncb = (uint64_t)mh_img * g.mw;            // Cb blocks of the image
    JPGE_HIP(launch_fdct(fdct_args(s, d.maxval, nullptr), s.stream));
    int16_t lastmcu[6 * 64];  // the stripe's last MCU: its Y11, Cb and Cr DCs seed the next stripe
    JPGE_HIP(hipMemcpyAsync(lastmcu, s.d_coef + ((size_t)g.nmcu() - 1) * 384, sizeof lastmcu, hipMemcpyDeviceToHost,
                            s.stream));
    JPGE_HIP(hipStreamSynchronize(s.stream));
    last_dc[0] = lastmcu[3 * 64];
    last_dc[1] = lastmcu[4 * 64];
    last_dc[2] = lastmcu[5 * 64];
    return kOk;
}

int Encoder::stripe_stats(const int32_t seed[3], uint32_t counts[1024], uint64_t first[1024]) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    Slot& s = slot0();
    if (!s.in.ptr || !seed || !counts || !first || huff_mode_) return kErrArg;
    for (int c = 0; c < 3; ++c) s.seed.v[c] = seed[c];
    const StatsArgs st = stats_args(s);
    JPGE_HIP(launch_stats(st, s.stream));
    s.seq = ++seq_counter_;
    s.hist = st.hist;
    if (const int e = export_hist(s)) return e;
    JPGE_HIP(hipStreamSynchronize(s.stream));
    read_hist(*s.h_hist, counts, first);
    return kOk;
}

EntropyArgs Encoder::stripe_entropy_args(Slot& s) {
    EntropyArgs e = entropy_args(s);
    e.done = nullptr;
    return e;
}

int Encoder::stripe_code(const uint32_t counts[1024], const uint64_t first[1024], StripeSummary* sum,
                         size_t* hdr_len) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    Slot& s = slot0();
    if (!s.in.ptr || !counts || !first || !sum || huff_mode_) return kErrArg;
    s.out_dev = nullptr;
    s.out_cap = 0;
    if (const int st = build_tables_from(s, counts, first, true)) return st;
    if (const int st = import_tables_copy(s)) return st;
    const EntropyArgs e = stripe_entropy_args(s);
    JPGE_HIP(launch_entropy_code_summary(e, s.stream));
    JPGE_HIP(hipMemcpyAsync(sum, e.summary, sizeof(StripeSummary), hipMemcpyDeviceToHost, s.stream));
    JPGE_HIP(hipStreamSynchronize(s.stream));
    if (hdr_len) *hdr_len = s.hdr_len;
    return kOk;
}

namespace {
uint32_t split_bits(uint32_t ptail, uint32_t head, uint32_t b) {  // 0 < b < 8 (entropy.hip)
    return (((ptail & ((1u << b) - 1)) << (8 - b)) | ((head & 0xFF) >> b)) & 0xFF;
}
uint32_t fill_bits(uint32_t eb, uint32_t tail) {  // Bitstream::fill, BitstreamGeneric.hpp:243-248
    return (((tail & ((1u << eb) - 1)) << (8 - eb)) | (0xFFu >> eb)) & 0xFF;
}
}  // namespace

int Encoder::stripe_place(const StripeSummary* all, int n, int index, size_t hdr_len, uint64_t* p_ext,
                          uint64_t* q_ext, uint32_t* head_split, size_t* seg_off, size_t* total_len) {
    if (!all || n <= 0 || index < 0 || index >= n) return kErrArg;
    if (all[0].restart) {  // restart stripes: self-contained byte runs, one after another
        uint64_t base = 0;
        for (int r = 0; r < n; ++r) {
            if (!all[r].restart) return kErrArg;
            if (r == index) {
                if (p_ext) *p_ext = 0;
                if (q_ext) *q_ext = base;  // (the byte base of the stripe after the header)
                if (head_split) *head_split = 0;
                if (seg_off) *seg_off = r == 0 ? 0 : hdr_len + (size_t)base;
            }
            base += all[r].bits;
        }
        if (total_len) *total_len = hdr_len + (size_t)base + 2;
        return kOk;
    }
    uint64_t p = 0, q = 0;
    for (int r = 0; r < n; ++r) {
        if (all[r].bits < 8) return kErrArg;  // (a stripe codes >= 2 bits per block, 6 blocks per MCU)
        const uint32_t b = (uint32_t)(p & 7);
        const uint32_t split = (b && r > 0) ? split_bits(all[r - 1].tail, all[r].head, b) : 0u;
        if (r == index) {
            if (p_ext) *p_ext = p;
            if (q_ext) *q_ext = q;
            if (head_split) *head_split = split;
            if (seg_off) *seg_off = r == 0 ? 0 : hdr_len + (size_t)(p >> 3) + (size_t)q;
        }
        // 0xFF bytes stripe r owns: its inside bytes at its alignment, the byte it
        // shares with its predecessor, the image's 1-filled final byte
        q += all[r].ff[b] + ((b && r > 0 && split == 0xFF) ? 1u : 0u);
        p += all[r].bits;
        if (r == n - 1 && (p & 7) && fill_bits((uint32_t)(p & 7), all[r].tail) == 0xFF) q += 1;
    }
    if (total_len) *total_len = hdr_len + (size_t)((p + 7) >> 3) + (size_t)q + 2;
    return kOk;
}

int Encoder::stripe_pack(const StripeSummary* all, int n, int index, uint8_t* out_dev, size_t cap, size_t* seg_off,
                         size_t* seg_len, size_t* total_len) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    Slot& s = slot0();
    if (!s.in.ptr || !out_dev || !s.hdr_len || huff_mode_) return kErrArg;
    uint64_t p_ext = 0, q_ext = 0;
    uint32_t head = 0;
    size_t off = 0, total = 0;
    if (const int st = stripe_place(all, n, index, s.hdr_len, &p_ext, &q_ext, &head, &off, &total)) return st;
    if (total > cap) return kErrNoSpace;
    s.out_dev = out_dev;
    s.out_cap = cap;
    s.seq = ++seq_counter_;
    s.h_result[2] = 0;
    EntropyArgs e = stripe_entropy_args(s);
    if (s.rst.mcus) {
        e.out_base = q_ext;  // (placed in phase 3, relative to the stripe's start)
    } else {
        e.p_ext = p_ext;
        e.q_ext = q_ext;
        e.head_split = head;
    }
    e.flags = (index == 0 ? kStripeFirst : 0u) | (index == n - 1 ? kStripeLast : 0u) | kExtPlace;
    JPGE_HIP(launch_entropy_place_pack(e, s.stream));
    if (const int w = wait_seq(&s.h_result[3], s.seq, s.stream)) return w;
    JPGE_HIP(hipStreamSynchronize(s.stream));
    if (s.h_result[1] & 4) return kErrNoSpace;
    const size_t end = (size_t)s.h_result[0];
    if (seg_off) *seg_off = off;
    if (seg_len) *seg_len = end - off;
    if (total_len) *total_len = total;
    return (index == n - 1 && end != total) ? kErrInternal : kOk;
}

}  // namespace jpge
