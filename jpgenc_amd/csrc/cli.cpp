// jpgenc — CLI with the reference's contract (src/main.cpp:8-32):
//   jpgenc <in.ppm> [out.jpg]      default output "noname.jpg"; no arguments
//                                  prints "No filename was written" and exits 0.
// Extensions: -q <1..100> (IJG-scaled tables, 50 = reference), JPGE_DEVICE=<n>;
//   --gpus N / --devices a,b,...   one image row-striped over a device group
//                                  (jpge_group_encode_striped: RCCL between distinct
//                                  devices), e.g. a 16384^2 frame over 8 GPUs;
//   --restart M                    restart interval in MCUs (DRI/RSTn);
//   --huffman optimal|standard     per-image Huffman tables (the default, the reference's
//                                  stream) or the ITU T.81 Annex K tables
//                                  (jpge_set_huffman; not with --gpus / --devices);
//   --downscale 2|4                code the image at 1/2 or 1/4 size, each sample the mean of
//                                  2x2 or 4x4 source samples (jpge_set_downscale; not with
//                                  --gpus / --devices);
//   --orient none|flip-h|rot180|flip-v|transpose|rot90|transverse|rot270
//                                  code the image flipped, rotated (rot90: clockwise) or
//                                  transposed (jpge_set_orientation; not with --gpus /
//                                  --devices, nor with --downscale 2|4);
//   --lut FILE                     map every sample through per-channel lookup tables: FILE holds
//                                  exactly 768 raw bytes, the R, G and B tables of 256 entries
//                                  (jpge_set_channel_lut; a PPM of maxval 255; not with --gpus /
//                                  --devices, --downscale 2|4 nor an --orient other than none).
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "jpge_image.hpp"

namespace {
int striped(const std::vector<int>& devs, const std::string& in, const std::string& out, int quality,
            uint32_t restart) {
    std::ifstream f(in, std::ios::binary);
    if (!f.is_open()) throw std::runtime_error("Failed to open \"" + in + "\"");
    std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    uint32_t w = 0, h = 0;
    int mv = 0;
    jpge::detail::check(jpge_ppm_info(buf.data(), buf.size(), &w, &h, &mv), "loadPPM");
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    jpge::detail::check(jpge_parse_ppm(buf.data(), buf.size(), rgb.data(), rgb.size(), &w, &h, &mv), "loadPPM");
    uint8_t qy[64], qc[64];
    jpge::detail::check(jpge_quality_tables(quality, qy, qc), "quality");
    jpge_group* g = nullptr;
    jpge::detail::check(jpge_group_open((int)devs.size(), devs.data(), 1, &g), "jpge_group_open");
    std::vector<uint8_t> jpg(jpge_max_jpeg_bytes(w, h));
    size_t len = 0;
    int st = jpge_group_set_restart_interval(g, restart);
    if (!st) st = jpge_group_encode_striped(g, rgb.data(), w, h, 0, mv, qy, qc, jpg.data(), jpg.size(), &len);
    jpge_group_close(g);
    jpge::detail::check(st, "jpge_group_encode_striped");
    std::ofstream o(out, std::ios::binary);
    if (!o.is_open()) throw std::runtime_error("Failed to open \"" + out + "\"");
    o.write(reinterpret_cast<const char*>(jpg.data()), (std::streamsize)len);
    return 0;
}
}  // namespace

int main(int argc, char* argv[]) {
    std::vector<std::string> pos;
    std::vector<int> devs;
    int quality = 50;
    uint32_t restart = 0;
    int huffman = JPGE_HUFF_OPTIMAL;
    int downscale = 1;
    int orient = JPGE_ORIENT_NONE;
    std::vector<uint8_t> lut;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "-q") && i + 1 < argc) {
            quality = std::atoi(argv[++i]);
        } else if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) {
            const int n = std::atoi(argv[++i]);
            devs.clear();
            for (int d = 0; d < n; ++d) devs.push_back(d);
        } else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) {
            devs.clear();
            std::stringstream ss(argv[++i]);
            std::string t;
            while (std::getline(ss, t, ',')) devs.push_back(std::atoi(t.c_str()));
        } else if (!std::strcmp(argv[i], "--restart") && i + 1 < argc) {
            restart = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
        } else if (!std::strcmp(argv[i], "--huffman") && i + 1 < argc) {
            const std::string m = argv[++i];
            if (m == "optimal") huffman = JPGE_HUFF_OPTIMAL;
            else if (m == "standard") huffman = JPGE_HUFF_STANDARD;
            else {
                std::cerr << "jpgenc: --huffman takes optimal or standard" << std::endl;
                return 1;
            }
        } else if (!std::strcmp(argv[i], "--downscale") && i + 1 < argc) {
            downscale = std::atoi(argv[++i]);
            if (downscale != 1 && downscale != 2 && downscale != 4) {
                std::cerr << "jpgenc: --downscale takes 1, 2 or 4" << std::endl;
                return 1;
            }
        } else if (!std::strcmp(argv[i], "--orient") && i + 1 < argc) {
            static const char* const names[8] = {"none", "flip-h", "rot180", "flip-v", "transpose", "rot90", "transverse", "rot270"};
            const std::string m = argv[++i];
            orient = -1;
            for (int o = 0; o < 8; ++o)
                if (m == names[o]) orient = o;
            if (orient < 0) {
                std::cerr << "jpgenc: --orient takes none, flip-h, rot180, flip-v, transpose, rot90, transverse or rot270" << std::endl;
                return 1;
            }
        } else if (!std::strcmp(argv[i], "--lut") && i + 1 < argc) {
            std::ifstream f(argv[++i], std::ios::binary);
            if (f.is_open()) lut.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            if (lut.size() != 768) {
                std::cerr << "jpgenc: --lut takes a file of exactly 768 bytes (the R, G and B tables)" << std::endl;
                return 1;
            }
        } else {
            pos.emplace_back(argv[i]);
        }
    }
    if (pos.empty()) {
        std::cout << "No filename was written" << std::endl;
        return 0;
    }
    const std::string jpg = pos.size() < 2 ? "noname.jpg" : pos[1];
    try {
        if (!devs.empty()) {
            if (huffman != JPGE_HUFF_OPTIMAL) throw std::runtime_error("--huffman standard: not for striped encodes");
            if (downscale != 1) throw std::runtime_error("--downscale: not for striped encodes");
            if (orient != JPGE_ORIENT_NONE) throw std::runtime_error("--orient: not for striped encodes");
            if (!lut.empty()) throw std::runtime_error("--lut: not for striped encodes");
            return striped(devs, pos[0], jpg, quality, restart);
        }
        auto img = jpge::loadPPM(pos[0]);
        if (restart) jpge::detail::check(jpge_set_restart_interval(jpge::default_context(), restart), "restart");
        if (huffman) jpge::detail::check(jpge_set_huffman(jpge::default_context(), huffman, nullptr), "huffman");
        if (downscale != 1) jpge::detail::check(jpge_set_downscale(jpge::default_context(), downscale), "downscale");
        if (orient != JPGE_ORIENT_NONE) jpge::detail::check(jpge_set_orientation(jpge::default_context(), orient), "orient");
        if (!lut.empty()) jpge::detail::check(jpge_set_channel_lut(jpge::default_context(), lut.data()), "lut");
        img.writeJPEG(jpg, quality);
    } catch (const std::exception& e) {
        std::cerr << "jpgenc: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
