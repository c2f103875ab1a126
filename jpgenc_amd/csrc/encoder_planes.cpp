// The Encoder's plane stages (the facade's Image stage methods on fp64 planes;
// planes.hip) and writeJPEG on planes.
#include "encoder_impl.hpp"

#include <cmath>

namespace jpge {

void* Encoder::scratch(int i, size_t bytes) {
    if ((int)scratch_.size() <= i) scratch_.resize(i + 1, {nullptr, 0});
    auto& b = scratch_[i];
    if (b.second < bytes) {
        hipFree(b.first);
        b = {nullptr, 0};
        if (hipMalloc(&b.first, bytes) != hipSuccess) return nullptr;
        b.second = bytes;
    }
    return b.first;
}

// A stage call's buffers: the caller's own where they are device buffers
// (kFlagDeviceInput / kFlagDeviceOutput), else the context's scratch buffer `index`,
// with host inputs copied in as they are named and the results copied out by finish().
// A failure is kept in `status` (the pointer returned is then null): check it once,
// before the launch.
struct Encoder::Staging {
    Encoder& enc;
    hipStream_t stream;
    uint32_t flags;
    int status = kOk;
    struct { void* host; const void* dev; size_t bytes; } owed[3] = {};
    int nowed = 0;

    template <class T>
    const T* in(int index, const T* p, size_t bytes) {
        if (flags & kFlagDeviceInput) return p;
        void* b = enc.scratch(index, bytes);
        if (!b || hipMemcpyAsync(b, p, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) {
            status = kErrHip;
            return nullptr;
        }
        return static_cast<const T*>(b);
    }
    template <class T>
    T* out(int index, T* p, size_t bytes) {
        if (flags & kFlagDeviceOutput) return p;
        void* b = enc.scratch(index, bytes);
        if (!b) status = kErrHip;
        else owed[nowed++] = {p, b, bytes};
        return static_cast<T*>(b);
    }
    int finish() {
        for (int i = 0; i < nowed; ++i)
            JPGE_HIP(hipMemcpyAsync(owed[i].host, owed[i].dev, owed[i].bytes, hipMemcpyDeviceToHost, stream));
        JPGE_HIP(hipStreamSynchronize(stream));
        return kOk;
    }
};

static PlaneColorArgs color_args(const double* const in[3], double* const out[3], size_t n, int to_ycc) {
    PlaneColorArgs a;
    a.in0 = in[0]; a.in1 = in[1]; a.in2 = in[2];
    a.out0 = out[0]; a.out1 = out[1]; a.out2 = out[2];
    a.n = n;
    a.to_ycc = to_ycc;
    return a;
}

int Encoder::stage_color(const double* const in[3], double* const out[3], size_t n, int to_ycc, uint32_t flags) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    for (int c = 0; c < 3; ++c)
        if (!in[c] || !out[c]) return kErrArg;
    if (n == 0) return kOk;
    Staging stg{*this, slot0().stream, flags};
    const double* din[3];
    double* dout[3];
    for (int c = 0; c < 3; ++c) {
        din[c] = stg.in(c, in[c], n * 8);
        dout[c] = stg.out(3 + c, out[c], n * 8);
    }
    if (stg.status) return stg.status;
    JPGE_HIP(launch_plane_color(color_args(din, dout, n, to_ycc), stg.stream));
    return stg.finish();
}

// applySubsampling's masks (Image.cpp:256-309) as PlaneSubsampleArgs; S444 leaves
// the plane as it is.
static bool subsample_mask(int mode, PlaneSubsampleArgs& a, uint32_t& vdiv) {
    a.mask[0] = 1; a.mask[1] = 0; a.mask[2] = 0; a.mask[3] = 0;
    a.m = 2; a.row_step = 2; a.avg_div = 0; vdiv = 2;
    switch (mode) {
        case 444: a.m = 1; a.row_step = 1; vdiv = 1; return true;
        case 422: a.row_step = 1; vdiv = 1; return true;               // {1, 0}
        case 411: a.m = 4; a.row_step = 1; vdiv = 1; return true;      // {1, 0, 0, 0}
        case 4200: return true;                                         // {1, 0}, scanline jump
        case 420: a.mask[1] = 1; a.avg_div = 4; return true;           // {1, 1}, averaging / 4
        case 4201: a.avg_div = 2; return true;                         // {1, 0}, averaging / 2
        default: return false;
    }
}

int Encoder::subsample_shape(int mode, uint32_t rows, uint32_t cols, uint32_t* out_rows, uint32_t* out_cols) {
    PlaneSubsampleArgs a;
    uint32_t vdiv;
    if (!subsample_mask(mode, a, vdiv)) return kErrArg;
    // the reference's loop reads whole mask runs and, in pairs, the next scanline
    if (rows == 0 || cols == 0 || cols % a.m || (a.row_step == 2 && rows % 2)) return kErrArg;
    if (out_rows) *out_rows = rows / vdiv;
    if (out_cols) *out_cols = cols / a.m;
    return kOk;
}

// a plane of rows x cols (a shape subsample_shape accepts) through `mode`'s mask
static PlaneSubsampleArgs subsample_args(int mode, const double* in, uint32_t rows, uint32_t cols, double* out) {
    PlaneSubsampleArgs a;
    uint32_t vdiv;
    subsample_mask(mode, a, vdiv);
    a.in = in;
    a.out = out;
    a.cols = cols;
    a.out_rows = rows / vdiv;
    a.out_cols = cols / a.m;
    return a;
}

int Encoder::stage_subsample(const double* in, uint32_t rows, uint32_t cols, int mode, double* out, uint32_t flags) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    uint32_t orows, ocols;
    if (!in || !out) return kErrArg;
    if (const int e = subsample_shape(mode, rows, cols, &orows, &ocols)) return e;
    Staging stg{*this, slot0().stream, flags};
    const size_t ib = (size_t)rows * cols * 8;
    const double* din = stg.in(0, in, ib);
    double* dout = stg.out(1, out, (size_t)orows * ocols * 8);
    if (stg.status) return stg.status;
    if (mode == 444) JPGE_HIP(hipMemcpyAsync(dout, din, ib, hipMemcpyDeviceToDevice, stg.stream));
    else JPGE_HIP(launch_plane_subsample(subsample_args(mode, din, rows, cols, dout), stg.stream));
    return stg.finish();
}

// Dct.hpp:220-235: A(k, n) = C0(k) sqrt(2/8) cos((2n+1) (k pi / 16)), glibc cos on the host
static void dct_matrix_a(double A[64]) {
    const double pi = 0x1.921fb54442d18p+1, root_two = 0x1.6a09e667f3bcdp+0;
    const double scale = std::sqrt(2. / 8);
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n) {
            const double cos_term = (2. * n + 1.) * ((k * pi) / (2. * 8));
            A[k * 8 + n] = (k == 0 ? 1. / root_two : 1.) * scale * std::cos(cos_term);
        }
}

int Encoder::stage_dct(const double* in, uint32_t rows, uint32_t cols, int dct_mode, double* out, uint32_t flags) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    if (!in || !out || rows % 8 || cols % 8 || dct_mode < kDctSimple || dct_mode > kDctArai) return kErrArg;
    if (rows == 0 || cols == 0) return kOk;
    Staging stg{*this, slot0().stream, flags};
    const size_t bytes = (size_t)rows * cols * 8;
    PlaneBlockArgs a{};
    a.in0 = stg.in(0, in, bytes);
    a.out_d = stg.out(1, out, bytes);
    if (stg.status) return stg.status;
    a.cols = cols;
    a.nblocks = (uint64_t)(rows / 8) * (cols / 8);
    a.sink = kSinkDouble;
    dct_matrix_a(a.A);
    JPGE_HIP(launch_plane_block(a, dct_mode, stg.stream));
    return stg.finish();
}

int Encoder::stage_quantize(const double* in, uint32_t rows, uint32_t cols, const uint8_t table[64], int32_t* out,
                            uint32_t flags) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    if (!in || !out || !table || rows % 8 || cols % 8) return kErrArg;
    if (rows == 0 || cols == 0) return kOk;
    Staging stg{*this, slot0().stream, flags};
    const size_t n = (size_t)rows * cols;
    PlaneQuantArgs a;
    a.in = stg.in(0, in, n * 8);
    a.out = stg.out(1, out, n * 4);
    if (stg.status) return stg.status;
    a.rows = rows;
    a.cols = cols;
    for (int i = 0; i < 64; ++i) a.q[i] = table[i];
    JPGE_HIP(launch_plane_quant(a, stg.stream));
    return stg.finish();
}

int Encoder::encode_planes(const double* const planes[3], uint32_t rows, uint32_t cols, int ycc, uint32_t real_w,
                           uint32_t real_h, const uint8_t qy[64], const uint8_t qc[64], uint8_t* out, size_t cap,
                           size_t* len, uint32_t flags) {
    std::lock_guard<std::recursive_mutex> call_lock(call_mu_);
    JPGE_HIP(hipSetDevice(device_));
    for (int c = 0; c < 3; ++c)
        if (!planes[c]) return kErrArg;
    if (huff_mode_) return kErrArg;  // (writeJPEG's per-image tables only)
    if (!out || !len || !qy || !qc || rows == 0 || cols == 0 || rows % 16 || cols % 16 || rows > 65536 ||
        cols > 65536 || real_w == 0 || real_h == 0 || real_w > 65535 || real_h > 65535)
        return kErrArg;
    if (!tables_nonzero(qy, qc)) return kErrArg;
    Slot& s = slot0();
    hipStream_t st = s.stream;
    // the frame as writeJPEG sees it: S420_m MCUs over the planes (rows, cols already
    // whole MCUs: loadPPM pads to 16, Image.cpp:480-531); SOF0 carries the real size
    Geometry g = geometry(cols, rows, 420);
    const bool dev_out = (flags & kFlagDeviceOutput) != 0;
    if (const int e = ensure(s, g, 0, dev_out ? 0 : max_jpeg_bytes(cols, rows))) return e;
    const size_t n = (size_t)rows * cols, bytes = n * 8;
    Staging stg{*this, st, flags};  // (the inputs only: the result is the slot's, finish()'s to deliver)
    const double* p[3];
    double* q[3] = {};  // the planes in YCbCr, when they come in RGB
    double* sub[2];     // the chroma planes at half size
    for (int c = 0; c < 3; ++c) p[c] = stg.in(c, planes[c], bytes);
    for (int c = 0; c < 3 && !ycc; ++c) q[c] = static_cast<double*>(scratch(3 + c, bytes));
    for (int c = 0; c < 2; ++c) sub[c] = static_cast<double*>(scratch(6 + c, bytes / 4));
    if (stg.status || (!ycc && (!q[0] || !q[1] || !q[2])) || !sub[0] || !sub[1]) return kErrHip;
    if (!ycc) {  // *this = convertToColorSpace(YCbCr), Image.cpp:839
        JPGE_HIP(launch_plane_color(color_args(p, q, n, 1), st));
        for (int c = 0; c < 3; ++c) p[c] = q[c];
    }
    // applySubsampling(S420_m), Image.cpp:842 (Cr, then Cb: independent planes)
    for (int c = 0; c < 2; ++c) JPGE_HIP(launch_plane_subsample(subsample_args(420, p[1 + c], rows, cols, sub[c]), st));
    // (the input pointer marks the slot in use; K1 is not run)
    FrameInput in;
    in.ptr = reinterpret_cast<const uint8_t*>(p[0]);
    s.begin(g, qy, qc, in, dev_out ? out : s.d_out, dev_out ? cap : s.cap_out, restart_mcus_, real_w, real_h);
    // applyDCT(Arai) + applyQuantization (Image.cpp:844-871) into the MCU layout; the
    // control block is zeroed here (K1 does it on the RGB8 path)
    const CtlLayout L(layout(g).grid());
    JPGE_HIP(hipMemsetAsync(s.d_ctl, 0, L.total, st));
    PlaneBlockArgs b{};
    b.in0 = p[0];
    b.in1 = sub[0];
    b.in2 = sub[1];
    b.cols = cols;
    b.nblocks = (uint64_t)g.nblocks();
    b.mcu = 1;
    b.sink = kSinkMcu16;
    for (int i = 0; i < 64; ++i) {
        b.q[i] = qy[i];
        b.q[64 + i] = qc[i];
    }
    b.out_h = s.d_coef;
    JPGE_HIP(launch_plane_block(b, kDctArai, st));
    const StatsArgs st2 = stats_args(s);
    JPGE_HIP(launch_stats(st2, st));
    s.seq = ++seq_counter_;
    s.hist = st2.hist;
    if (const int e = export_hist(s)) return e;
    FrameDesc f;
    f.out = out;
    f.cap = cap;
    int e = build_tables(s, false);
    if (!e) e = import_tables_copy(s);
    if (!e) e = launch_entropy_phase(s, nullptr);
    if (!e) e = finish(s, f, flags);
    hipStreamSynchronize(st);
    *len = f.len;
    return e;
}

}  // namespace jpge
