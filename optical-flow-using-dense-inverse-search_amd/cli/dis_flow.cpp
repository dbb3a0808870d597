// dis_flow -- frame-sequence CLI over the MI355X engine,
// the reference's main() (src/main.cpp:59-206) with its argument conventions:
//
//   dis_flow                                   alley_1 frames 1..50, defaults (the usage, if ./alley_1 is absent)
//   dis_flow folder start end
//   dis_flow folder start end iters patch_size coarsest finest overlap norm draw_grid
//
// plus options (after the positionals): --flo (also write OF_<folder>/frame_NNNN.flo,
// the SaveFlowFile format of src/IO_flow.cpp:56-98, which the reference left
// commented out at src/main.cpp:137-146), --batch N (pairs per GPU call,
// default 8; the reference is one pair at a time), --device D, --paper (the DIS
// paper's residual and densification; not the reference's),
// --refine K (K fixed-point iterations of variational refinement, 8f row 1),
// --bidir (both directions in one GPU call: also writes the backward flow's
// colour coding OF_<folder>/frame_NNNN_bw.png -- and frame_NNNN_bw.flo with
// --flo -- and the forward flow's forward-backward consistency mask as the
// 8-bit grey frame_NNNN_mask.png, 255 = consistent), --fb-alpha A1 A2 (the
// check's constants, default 0.01 0.5), --warm-start (temporal warm start: each
// pair's search starts from the previous pair's flow, the first pair from zero;
// one pair per GPU call, so it is refused together with --batch N > 1 and with
// --bidir -- the pairs of one batch run concurrently and have no previous flow),
// --warp (also write OF_<folder>/frame_NNNN_warp.png: the pair's second frame
// warped back by the computed -- with --bidir, the forward -- flow, 8-bit grey,
// targets outside the frame clamped; and print the mean absolute difference to
// the first frame over the pixels whose target lies inside the frame, next to
// the unwarped second frame's), --interp K (also write
// OF_<folder>/frame_NNNN_interp_k.png for k = 1..K: the frame at time
// t = k / (K + 1) between the pair's two frames, 8-bit grey, interpolated with
// the computed flow by dis::flowInterp; holes are filled from the backward flow
// with --bidir, from the forward flow alone without), --color (the frames are
// read as 8-bit RGB, png::read_rgb, and handed to the engine as they are: it
// runs with DIS_FRAME_RGB8 and reduces them to gray on the GPU by the luma that
// the PNG reader applies without --color, so flows, .flo files and colour-coded
// images are the same bytes either way; --warp and --interp then run on the
// three-channel frames and write colour PNGs, and --warp's mean absolute
// differences are taken over all samples of the valid pixels), --accumulate (the
// pair flows are chained by dis::flowCompose into the flow from frame `start`
// to each pair's second frame: the first pair's flow itself, then composed with
// every later pair's in order -- after each batch with --batch N -- carrying
// the valid map along; with --bidir pair k's forward consistency mask gates
// its taps (mask_b). With --flo it is written as
// OF_<folder>/frame_NNNN_acc.flo, invalid vectors as NaN; the count of valid
// pixels is printed either way), --fill (needs --bidir: the forward flow's
// vectors that fail the consistency check are replaced by dis::flowFill's
// push-pull from those that pass; also writes OF_<folder>/frame_NNNN_filled.flo
// and the level each vector came from as the 8-bit grey frame_NNNN_fill.png, 0 =
// kept. With --accumulate the accumulated field is filled after each
// composition, its valid map as the mask, and goes on with every pixel valid;
// the count line then also gives the number of filled pixels), --motion MODEL
// (MODEL = translation, similarity or affine: the pair's global motion by
// dis::fitMotion with its defaults, three refits within 1 px, written as
// OF_<folder>/frame_NNNN_motion.txt: one line of the six parameters p0 .. p5,
// u = p0 + p1 x + p2 y and v = p3 + p4 x + p5 y, "%.9g" each, nan where the fit
// failed; with --bidir only the vectors that pass the consistency check are
// fitted), --denoise R SIGMA (after the pairs: every frame start .. end is
// denoised in time by dis::temporalDenoise from the up to 2 R frames within R of
// it that the range holds -- the end frames have fewer --, each warped to it by
// the flow from it to that frame, which comes from the same engine in calls of
// up to N pairs, with the table dis::denoiseWeights(SIGMA) and no masks; R in
// [1, 4], SIGMA about 1.5 times the noise's standard deviation. Written as
// OF_<folder>/frame_NNNN_denoised.png, 8-bit grey, colour with --color),
// --stabilize R (after the pairs: the pair models of the range -- --motion's
// MODEL, similarity without it, fitted as above -- go through dis::stabilizePath
// with radius R in [0, 1024], sigma max(R, 1) / 2 and --stab-zoom Z's zoom (1 by
// default, up to 16), and every frame start .. end is warped by its correction
// with dis::warpMotion, up to N frames a call. Written as
// OF_<folder>/frame_NNNN_stab.png, 8-bit grey, colour with --color; the
// corrections, one "%.9g" line per frame, as OF_<folder>/stab_corrections.txt),
// --homography (the pair's global motion as a homography by dis::fitHomography
// with its defaults, written as OF_<folder>/frame_NNNN_homography.txt: one line
// of the eight parameters p0 .. p7, "%.9g" each, nan where the fit failed; with
// --bidir only the consistent vectors are fitted; and --stabilize R then runs
// the homography chain: these pair models through dis::stabilizePathHomography
// and dis::warpHomography, eight values a line in stab_corrections.txt;
// --motion's names and files are as without it).
//
// For img_i in [start, end): reads <folder>/frame_<img_i>.png and frame_<img_i+1>
// (grayscale, src/main.cpp:118-130), computes the full-resolution flow
// (dis::DenseInverseSearch::calc: src/main.cpp:135-198), colour-codes it
// (dis_flow_color = draw_optical_flow, :200) and writes OF_<folder>/frame_<img_i>.png
// (:201). GUI windows (imshow / draw_grid) are not supported.
#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "dis/dis.hpp"
#include "png.hpp"

namespace {

std::string frame_name(const std::string& folder, int i)
{
    char buf[32];
    std::snprintf(buf, sizeof buf, "/frame_%04d", i);
    return folder + buf;
}

void usage()
{
    std::cout << "Not good parameters!\n"
                 "1. Run without parameters with default parameters (alley_1) from 1 to 50\n"
                 "2. Set folder and images with default parameters:\n"
                 "dis_flow folder start_num_image end_num_image\n"
                 "3. Add full settings\n"
                 "dis_flow folder start_num_image end_num_image max_iter patch_size coarsest_scale finest_scale "
                 "patch_overlap patch_norm draw_grid\n"
                 "options: --flo  --batch N  --device D  --paper  --refine K  --bidir  --fb-alpha A1 A2  --warm-start  --warp  "
                 "--interp K  --color  --accumulate  --fill  --motion MODEL  --denoise R SIGMA  "
                 "--stabilize R  --stab-zoom Z  --homography"
              << std::endl;
}

}  // namespace

int main(int argc, char** argv)
{
    // reference defaults, src/main.cpp:63-72
    std::string folder = "alley_1";
    int start = 1, end = 50;
    dis_params p{};
    p.iterations = 1000;
    p.patch_size = 8;
    p.coarsest_scale = 3;
    p.finest_scale = 0;
    p.patch_overlap = 0.7f;
    p.patch_normalization = 1;
    p.var_refine_iters = 0;
    int draw_grid = 0;
    bool write_flo = false;
    int batch = 8, device = 0;
    bool bidir = false, warm_start = false, batch_given = false, warp = false;
    float fb_alpha1 = 0.01f, fb_alpha2 = 0.5f;
    int interp = 0;
    bool color = false, accumulate = false, fill = false;
    bool homography = false;  // --homography: the eight-parameter fit, and --stabilize's chain by it
    std::string motion;  // --motion: the model's name (empty: no fit)
    int denoise = 0;     // --denoise: the radius R (0: off)
    float denoise_sigma = 0.0f;
    bool denoise_given = false;
    int stabilize = 0;  // --stabilize: the radius R
    bool stabilize_given = false;
    float stab_zoom = 1.0f;

    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--flo") {
            write_flo = true;
        } else if (a == "--batch" && i + 1 < argc) {
            batch = std::atoi(argv[++i]);
            batch_given = true;
        } else if (a == "--device" && i + 1 < argc) {
            device = std::atoi(argv[++i]);
        } else if (a == "--bidir") {
            bidir = true;
        } else if (a == "--warm-start") {
            warm_start = true;
        } else if (a == "--warp") {
            warp = true;
        } else if (a == "--color") {
            color = true;
        } else if (a == "--accumulate") {
            accumulate = true;
        } else if (a == "--fill") {
            fill = true;
        } else if (a == "--homography") {
            homography = true;
        } else if (a == "--motion" && i + 1 < argc) {
            motion = argv[++i];
        } else if (a == "--denoise" && i + 2 < argc) {
            denoise = std::atoi(argv[++i]);
            denoise_sigma = (float)std::atof(argv[++i]);
            denoise_given = true;
        } else if (a == "--stabilize" && i + 1 < argc) {
            stabilize = std::atoi(argv[++i]);
            stabilize_given = true;
        } else if (a == "--stab-zoom" && i + 1 < argc) {
            stab_zoom = (float)std::atof(argv[++i]);
        } else if (a == "--interp" && i + 1 < argc) {
            interp = std::atoi(argv[++i]);
        } else if (a == "--fb-alpha" && i + 2 < argc) {
            fb_alpha1 = (float)std::atof(argv[++i]);
            fb_alpha2 = (float)std::atof(argv[++i]);
        } else if (a == "--paper") {
            p.paper_mode = 1;
        } else if (a == "--refine" && i + 1 < argc) {
            p.var_refine_iters = std::atoi(argv[++i]);
        } else {
            pos.push_back(a);
        }
    }
    if (pos.size() == 3 || pos.size() == 10) {
        folder = pos[0];
        start = std::atoi(pos[1].c_str());
        end = std::atoi(pos[2].c_str());
    }
    if (pos.size() == 10) {  // argv[4..10] order of src/main.cpp:84-92
        p.iterations = std::atoi(pos[3].c_str());
        p.patch_size = std::atoi(pos[4].c_str());
        p.coarsest_scale = std::atoi(pos[5].c_str());
        p.finest_scale = std::atoi(pos[6].c_str());
        p.patch_overlap = (float)std::atof(pos[7].c_str());
        p.patch_normalization = std::atoi(pos[8].c_str());
        draw_grid = std::atoi(pos[9].c_str());
    } else if (!pos.empty() && pos.size() != 3) {
        usage();
        return 0;  // as the reference
    }
    if (draw_grid) {
        std::cerr << "draw_grid (OpenCV GUI) is not supported" << std::endl;
        return 2;
    }
    if (batch < 1) batch = 1;
    if (interp < 0 || interp > 99) {
        std::cerr << "--interp K: K must lie in [0, 99]" << std::endl;
        return 2;
    }
    if (denoise_given && (denoise < 1 || denoise > DIS_DENOISE_MAX_NEIGHBOURS / 2 || !(denoise_sigma > 0.0f) ||
                          !(denoise_sigma < 1e30f))) {
        std::cerr << "--denoise R SIGMA: R must lie in [1, 4] and SIGMA must be finite and > 0" << std::endl;
        return 2;
    }
    if (stabilize_given && (stabilize < 0 || stabilize > 1024 || !(stab_zoom >= 1.0f && stab_zoom <= 16.0f))) {
        std::cerr << "--stabilize R, --stab-zoom Z: R must lie in [0, 1024] and Z in [1, 16]" << std::endl;
        return 2;
    }
    if (warm_start && ((batch_given && batch > 1) || bidir)) {
        std::cerr << "--warm-start seeds each pair from the previous pair's flow: it cannot be combined with "
                  << (bidir ? "--bidir" : "--batch N > 1")
                  << " (the pairs of one batch run concurrently, so there is no previous flow)" << std::endl;
        return 2;
    }
    if (warm_start) batch = 1;
    if (fill && !bidir) {
        std::cerr << "--fill replaces the vectors that fail the forward-backward check: it needs --bidir" << std::endl;
        return 2;
    }
    dis::MotionModel motion_model = dis::MotionModel::AFFINE;
    if (motion == "translation") {
        motion_model = dis::MotionModel::TRANSLATION;
    } else if (motion == "similarity") {
        motion_model = dis::MotionModel::SIMILARITY;
    } else if (!motion.empty() && motion != "affine") {
        std::cerr << "--motion MODEL: MODEL must be translation, similarity or affine" << std::endl;
        return 2;
    }
    if (stabilize_given && motion.empty()) motion_model = dis::MotionModel::SIMILARITY;
    struct stat sb;
    if (argc == 1 && ::stat(folder.c_str(), &sb) != 0) {  // no arguments and no default sequence here
        usage();
        return 0;
    }
    const std::string out_dir = "OF_" + folder;
    ::mkdir(out_dir.c_str(), 0755);  // CreateFolder (src/main.cpp:52-57): existing is fine

    try {
        std::unique_ptr<dis::DenseInverseSearch> eng;
        int W = 0, H = 0;
        std::vector<float> prev_flow;  // --warm-start: the previous pair's flow (empty: start cold)
        std::vector<float> acc;        // --accumulate: the flow from frame `start` to the last pair's second frame
        std::vector<uint8_t> acc_valid;
        std::vector<float> pair_models;  // --stabilize: the six parameters of every pair of the range
        for (int i0 = start; i0 < end; i0 += batch) {
            const int n = std::min(batch, end - i0);
            struct Frame {
                int width, height;
                std::vector<uint8_t> px;  // width * height * C samples
            };
            const int C = color ? 3 : 1;  // samples per pixel of the frames
            std::vector<Frame> frames;
            for (int k = 0; k <= n; ++k) {
                if (k < n) std::cout << "start " << frame_name(folder, i0 + k) << ".png" << std::endl;
                const std::string path = frame_name(folder, i0 + k) + ".png";
                if (color) {
                    png::Rgb f = png::read_rgb(path);
                    frames.push_back({f.width, f.height, std::move(f.px)});
                } else {
                    png::Gray f = png::read_gray(path);
                    frames.push_back({f.width, f.height, std::move(f.px)});
                }
            }
            if (!eng || frames[0].width != W || frames[0].height != H) {
                W = frames[0].width;
                H = frames[0].height;
                eng.reset(new dis::DenseInverseSearch(p, W, H, batch, device));
                if (color) eng->set_frame_format(dis::FrameFormat::RGB8);
                prev_flow.clear();
                acc.clear();
            }
            const size_t fsz = (size_t)W * H * C;  // bytes of one frame
            std::vector<uint8_t> I0((size_t)n * fsz), I1((size_t)n * fsz);
            for (int k = 0; k < n; ++k) {
                if (frames[k].width != W || frames[k].height != H || frames[k + 1].width != W || frames[k + 1].height != H)
                    throw std::runtime_error("frame sizes differ within a batch");
                std::copy(frames[k].px.begin(), frames[k].px.end(), I0.begin() + (size_t)k * fsz);
                std::copy(frames[k + 1].px.begin(), frames[k + 1].px.end(), I1.begin() + (size_t)k * fsz);
            }
            auto write_frame = [&](const std::string& path, const uint8_t* px) {
                if (color)
                    png::write_rgb(path, px, W, H);
                else
                    png::write_gray(path, px, W, H);
            };
            std::vector<float> flow((size_t)n * W * H * 2);
            std::vector<float> flow_bw;
            std::vector<uint8_t> mask, bgr_bw;
            if (bidir) {
                flow_bw.resize(flow.size());
                mask.resize((size_t)n * W * H);
                bgr_bw.resize((size_t)n * W * H * 3);
                eng->calc_bidir_batch(n, I0.data(), I1.data(), flow.data(), flow_bw.data());
                dis::flowConsistency(flow.data(), flow_bw.data(), n, W, H, mask.data(), nullptr, fb_alpha1, fb_alpha2,
                                     DIS_MEM_HOST, nullptr, device);
                dis::check(dis_flow_color(flow_bw.data(), n, W, H, -1.0f, bgr_bw.data(), DIS_MEM_HOST, nullptr, device));
            } else if (warm_start) {
                eng->calc(I0.data(), I1.data(), flow.data(), prev_flow.empty() ? nullptr : prev_flow.data(),
                          dis::InitKind::FULLRES);
                prev_flow = flow;
            } else {
                eng->calc_batch(n, I0.data(), I1.data(), flow.data());
            }
            std::vector<float> filled;
            std::vector<uint8_t> fill_level;
            if (fill) {
                filled.resize(flow.size());
                fill_level.resize((size_t)n * W * H);
                dis::flowFill(flow.data(), n, W, H, filled.data(), mask.data(), fill_level.data(), nullptr, DIS_MEM_HOST,
                              nullptr, device);
            }
            std::vector<float> motion_params, homography_params;
            if (!motion.empty() || (stabilize_given && !homography)) {
                motion_params.resize((size_t)n * 6);
                dis::fitMotion(flow.data(), n, W, H, motion_params.data(), motion_model, 3, 1.0f,
                               bidir ? mask.data() : nullptr, nullptr, nullptr, nullptr, DIS_MEM_HOST, nullptr, device);
            }
            if (homography) {
                homography_params.resize((size_t)n * 8);
                dis::fitHomography(flow.data(), n, W, H, homography_params.data(), 3, 1.0f, bidir ? mask.data() : nullptr,
                                   nullptr, nullptr, nullptr, DIS_MEM_HOST, nullptr, device);
            }
            if (stabilize_given) {
                const std::vector<float>& m = homography ? homography_params : motion_params;
                pair_models.insert(pair_models.end(), m.begin(), m.end());
            }
            std::vector<uint8_t> bgr((size_t)n * W * H * 3);
            dis::check(dis_flow_color(flow.data(), n, W, H, -1.0f, bgr.data(), DIS_MEM_HOST, nullptr, device));
            std::vector<uint8_t> warped, inside;
            if (warp) {
                warped.resize((size_t)n * fsz);
                inside.resize((size_t)n * W * H);
                dis::flowWarp(I1.data(), C, flow.data(), n, W, H, warped.data(), 1.0f, dis::Border::REPLICATE,
                              inside.data(), 0, 0, DIS_MEM_HOST, nullptr, device);
            }
            std::vector<uint8_t> mid((size_t)n * fsz);
            for (int j = 1; j <= interp; ++j) {
                dis::flowInterp(I0.data(), I1.data(), C, flow.data(), bidir ? flow_bw.data() : nullptr, n, W, H,
                                (float)j / (float)(interp + 1), mid.data(), nullptr, nullptr, 0, 0, DIS_MEM_HOST,
                                nullptr, device);
                for (int k = 0; k < n; ++k)
                    write_frame("OF_" + frame_name(folder, i0 + k) + "_interp_" + std::to_string(j) + ".png",
                                mid.data() + (size_t)k * fsz);
            }
            for (int k = 0; k < n; ++k) {
                const std::string base = "OF_" + frame_name(folder, i0 + k);
                png::write_bgr(base + ".png", bgr.data() + (size_t)k * W * H * 3, W, H);
                if (warp) {
                    const size_t o = (size_t)k * W * H;
                    write_frame(base + "_warp.png", warped.data() + o * C);
                    long long cnt = 0, d_warp = 0, d_plain = 0;
                    for (size_t q = o; q < o + (size_t)W * H; ++q)
                        if (inside[q]) {
                            ++cnt;
                            for (size_t j = q * C; j < (q + 1) * C; ++j) {
                                d_warp += std::abs((int)warped[j] - (int)I0[j]);
                                d_plain += std::abs((int)I1[j] - (int)I0[j]);
                            }
                        }
                    const double samples = (double)cnt * C;
                    std::cout << "warp " << frame_name(folder, i0 + k) << ".png: mean |warped - first| "
                              << (cnt ? (double)d_warp / samples : 0.0) << ", mean |second - first| "
                              << (cnt ? (double)d_plain / samples : 0.0) << " over " << cnt << " valid pixels" << std::endl;
                }
                if (write_flo)
                    dis::check(dis_write_flo((base + ".flo").c_str(), flow.data() + (size_t)k * W * H * 2, W, H, 2));
                if (accumulate) {
                    const size_t px = (size_t)W * H;
                    if (acc.empty()) {  // the first pair: its flow is the accumulated one
                        acc.assign(flow.begin() + k * px * 2, flow.begin() + (k + 1) * px * 2);
                        acc_valid.assign(px, 255);
                    } else {  // in place: acc <- acc o flow_k
                        dis::flowCompose(acc.data(), flow.data() + k * px * 2, 1, W, H, acc.data(), acc_valid.data(),
                                         bidir ? mask.data() + k * px : nullptr, acc_valid.data(), DIS_MEM_HOST, nullptr,
                                         device);
                    }
                    size_t cnt = 0;
                    for (size_t q = 0; q < px; ++q) cnt += acc_valid[q] != 0;
                    std::cout << "accumulate " << frame_name(folder, i0 + k) << ".png: " << cnt << " of " << px
                              << " pixels followed from frame " << start;
                    if (fill) {  // in place: the untrusted vectors from the trusted ones, then all are valid
                        dis::flowFill(acc.data(), 1, W, H, acc.data(), acc_valid.data(), nullptr, nullptr, DIS_MEM_HOST,
                                      nullptr, device);
                        acc_valid.assign(px, 255);
                        std::cout << ", " << px - cnt << " filled";
                    }
                    std::cout << std::endl;
                    if (write_flo) dis::check(dis_write_flo((base + "_acc.flo").c_str(), acc.data(), W, H, 2));
                }
                if (!motion.empty()) {
                    const float* m = motion_params.data() + (size_t)k * 6;
                    char line[128];
                    std::snprintf(line, sizeof line, "%.9g %.9g %.9g %.9g %.9g %.9g\n", m[0], m[1], m[2], m[3], m[4], m[5]);
                    std::FILE* f = std::fopen((base + "_motion.txt").c_str(), "w");
                    if (!f || std::fputs(line, f) < 0 || std::fclose(f) != 0)
                        throw std::runtime_error("cannot write " + base + "_motion.txt");
                }
                if (homography) {
                    const float* m = homography_params.data() + (size_t)k * 8;
                    char line[192];
                    std::snprintf(line, sizeof line, "%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", m[0], m[1], m[2], m[3], m[4],
                                  m[5], m[6], m[7]);
                    std::FILE* f = std::fopen((base + "_homography.txt").c_str(), "w");
                    if (!f || std::fputs(line, f) < 0 || std::fclose(f) != 0)
                        throw std::runtime_error("cannot write " + base + "_homography.txt");
                }
                if (fill) {
                    dis::check(dis_write_flo((base + "_filled.flo").c_str(), filled.data() + (size_t)k * W * H * 2, W, H, 2));
                    png::write_gray(base + "_fill.png", fill_level.data() + (size_t)k * W * H, W, H);
                }
                if (bidir) {
                    png::write_bgr(base + "_bw.png", bgr_bw.data() + (size_t)k * W * H * 3, W, H);
                    png::write_gray(base + "_mask.png", mask.data() + (size_t)k * W * H, W, H);
                    if (write_flo)
                        dis::check(dis_write_flo((base + "_bw.flo").c_str(), flow_bw.data() + (size_t)k * W * H * 2, W,
                                                 H, 2));
                }
                std::cout << "finish " << frame_name(folder, i0 + k) << ".png" << std::endl;
            }
        }
        if (denoise && eng) {  // --denoise: every frame of the range from its neighbours in time
            const int C = color ? 3 : 1, T = end - start + 1;
            const size_t fsz = (size_t)W * H * C, vsz = (size_t)W * H * 2;
            std::vector<std::vector<uint8_t>> seq;
            for (int t = 0; t < T; ++t) {
                const std::string path = frame_name(folder, start + t) + ".png";
                int w, h;
                if (color) {
                    png::Rgb f = png::read_rgb(path);
                    w = f.width, h = f.height;
                    seq.push_back(std::move(f.px));
                } else {
                    png::Gray f = png::read_gray(path);
                    w = f.width, h = f.height;
                    seq.push_back(std::move(f.px));
                }
                if (w != W || h != H) throw std::runtime_error("--denoise: frame sizes differ within the range");
            }
            const std::vector<float> table = dis::denoiseWeights(denoise_sigma);
            std::vector<uint8_t> out(fsz);
            for (int t = 0; t < T; ++t) {
                std::vector<int> js;
                for (int j = std::max(t - denoise, 0); j <= std::min(t + denoise, T - 1); ++j)
                    if (j != t) js.push_back(j);
                const int K = (int)js.size();
                std::vector<float> flows((size_t)K * vsz);
                for (int b = 0; b < K; b += batch) {  // the flows from frame t to its neighbours, up to `batch` a call
                    const int n = std::min(batch, K - b);
                    std::vector<uint8_t> I0((size_t)n * fsz), I1((size_t)n * fsz);
                    for (int k = 0; k < n; ++k) {
                        std::copy(seq[t].begin(), seq[t].end(), I0.begin() + (size_t)k * fsz);
                        std::copy(seq[js[b + k]].begin(), seq[js[b + k]].end(), I1.begin() + (size_t)k * fsz);
                    }
                    eng->calc_batch(n, I0.data(), I1.data(), flows.data() + (size_t)b * vsz);
                }
                std::vector<const uint8_t*> nb;
                std::vector<const float*> fl;
                for (int k = 0; k < K; ++k) {
                    nb.push_back(seq[js[k]].data());
                    fl.push_back(flows.data() + (size_t)k * vsz);
                }
                dis::temporalDenoise(seq[t].data(), nb.data(), C, fl.data(), K, 1, W, H, table.data(), out.data(), nullptr,
                                     nullptr, 0, 0, DIS_MEM_HOST, nullptr, device);
                const std::string path = "OF_" + frame_name(folder, start + t) + "_denoised.png";
                if (color)
                    png::write_rgb(path, out.data(), W, H);
                else
                    png::write_gray(path, out.data(), W, H);
                std::cout << "denoised " << frame_name(folder, start + t) << ".png from " << K << " frames" << std::endl;
            }
        }
        if (stabilize_given && eng) {  // --stabilize: every frame of the range onto the smoothed camera path
            const int C = color ? 3 : 1, T = end - start + 1;
            const size_t fsz = (size_t)W * H * C;
            const int PM = homography ? 8 : 6;  // parameters of a model
            if (pair_models.size() != (size_t)(T - 1) * PM)
                throw std::runtime_error("--stabilize: the frame size changed within the range");
            const float stab_sigma = (float)std::max(stabilize, 1) / 2.0f;
            const std::vector<float> corr =
                homography ? dis::stabilizePathHomography(pair_models.data(), T, W, H, stabilize, stab_sigma, stab_zoom)
                           : dis::stabilizePath(pair_models.data(), T, W, H, stabilize, stab_sigma, stab_zoom);
            std::FILE* cf = std::fopen((out_dir + "/stab_corrections.txt").c_str(), "w");
            if (!cf) throw std::runtime_error("cannot write " + out_dir + "/stab_corrections.txt");
            for (int t = 0; t < T; ++t) {
                const float* m = corr.data() + (size_t)t * PM;
                std::fprintf(cf, "%.9g %.9g %.9g %.9g %.9g %.9g", m[0], m[1], m[2], m[3], m[4], m[5]);
                if (homography) std::fprintf(cf, " %.9g %.9g", m[6], m[7]);
                std::fprintf(cf, "\n");
            }
            if (std::fclose(cf) != 0) throw std::runtime_error("cannot write " + out_dir + "/stab_corrections.txt");
            for (int t0 = 0; t0 < T; t0 += batch) {
                const int n = std::min(batch, T - t0);
                std::vector<uint8_t> src((size_t)n * fsz), dst((size_t)n * fsz);
                for (int k = 0; k < n; ++k) {
                    const std::string path = frame_name(folder, start + t0 + k) + ".png";
                    int w, h;
                    std::vector<uint8_t> px;
                    if (color) {
                        png::Rgb f = png::read_rgb(path);
                        w = f.width, h = f.height, px = std::move(f.px);
                    } else {
                        png::Gray f = png::read_gray(path);
                        w = f.width, h = f.height, px = std::move(f.px);
                    }
                    if (w != W || h != H) throw std::runtime_error("--stabilize: frame sizes differ within the range");
                    std::copy(px.begin(), px.end(), src.begin() + (size_t)k * fsz);
                }
                if (homography)
                    dis::warpHomography(src.data(), C, corr.data() + (size_t)t0 * 8, n, W, H, dst.data(),
                                        dis::Border::REPLICATE, nullptr, 0, 0, DIS_MEM_HOST, nullptr, device);
                else
                    dis::warpMotion(src.data(), C, corr.data() + (size_t)t0 * 6, n, W, H, dst.data(), dis::Border::REPLICATE,
                                    nullptr, 0, 0, DIS_MEM_HOST, nullptr, device);
                for (int k = 0; k < n; ++k) {
                    const std::string path = "OF_" + frame_name(folder, start + t0 + k) + "_stab.png";
                    if (color)
                        png::write_rgb(path, dst.data() + (size_t)k * fsz, W, H);
                    else
                        png::write_gray(path, dst.data() + (size_t)k * fsz, W, H);
                    std::cout << "stabilised " << frame_name(folder, start + t0 + k) << ".png" << std::endl;
                }
            }
        }
    } catch (const std::exception& e) {
        std::cerr << "dis_flow: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
