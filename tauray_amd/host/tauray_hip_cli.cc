// tauray_hip - headless command line front-end of the MI355X path-tracing core, shaped after `tauray --headless`
// (reference src/main.cc, src/tauray.cc:1017-1132 replay_viewer): load a scene, create an rt_renderer over the
// selected devices, render N frames, tonemap, save.  Scene input is a .glb / .gltf file (include/tauray_gltf.hh, the loader of
// src/gltf.cc for the path tracer's subset) or a .trsc dump (tauray_amd/scene_io.py); --dump-scene=out.trsc writes the loaded
// scene as a dump and exits without touching a GPU.
//
//   tauray_hip scene.glb|scene.trsc --width=512 --height=512 --headless=out/frame [--max-ray-depth=8] [--samples-per-pixel=1]
//              [--frames=1] [--fake-devices=N | --devices=0,1,...] [--distribution-strategy=scanline|shuffled-strips]
//              [--filetype=exr|raw|none] [--format=rgb16|rgb32|rgba16|rgba32] [--tonemap=filmic|linear|gamma-correction|
//              reinhard|reinhard-luminance] [--exposure=1] [--gamma=2.2] [--sampler=uniform-random|sobol-owen|sobol-z2|sobol-z3]
//              [--rng-seed=0] [--accumulation] [-t] [--skip-nan-check] [--warmup-frames=0] [--frames-in-flight=1] [--frames-per-launch=1]
//              [--renderer=restir-di [--restir=candidates,spatial_samples,search_radius,max_confidence,temporal_reuse]]
//              [--restir-visibility=per-target|shared|sampled]   (with --renderer=restir-di and restir-gi)
//              [--restir-light-selection=uniform|power[,fraction]]   (with --renderer=restir-di and restir-gi)
//              [--restir-bsdf-candidates=N]   (with --renderer=restir-di and restir-gi)
//              [--restir-sphere-lights=point|area]   (with --renderer=restir-di and restir-gi)
//              [--renderer=restir-gi [--restir-gi=spatial_samples,search_radius,max_confidence,temporal_reuse] [--restir-gi-bounces=N] [--restir=...]]
//              [--renderer=path-tracer|direct|sh-probes|dshgi [--samples-per-probe=512] [--sh-order=2] [--dshgi-temporal-ratio=0.01]
//               [--use-probe-visibility] [--brdf-integration=FILE.exr]] [--denoiser=none|bmfr] [--spatial-reprojection=i,j,...] [--temporal-reprojection=r]
//              [--taa=N[,edge-dilation=on|off][,anti-shimmer=on|off]]
//              [--animation[=NAME] --framerate=F [--deformation-motion]]   (screen motion follows skinned and morphed meshes as they deform)
//              [--display=headless|looking-glass --lkg-params=viewports,midplane,depth,relative_dist
//               --lkg-calibration=display_index,pitch,slope,center,fringe,viewCone,invView,verticalAngle,DPI,screenW,screenH,flipImageX,flipImageY,flipSubp]
//              (a Looking Glass output: --width / --height are the size of one view, one composed screenW x screenH file per frame)
//              [--camera-grid=w,h,x,y --camera-recentering-distance=5 --camera-grid-roll=0]   (light-field grid, one file per view)
//
// One process per GPU (include/tauray_hip_comm.hh): start N copies with --process-count=N --process-rank=0..N-1 --device=<HIP index>
// --comm-id=<file on a shared file system> [--comm-nonce=<number every rank of this job gets, e.g. the launcher's pid>] (rank 0 writes the RCCL id
// there under that nonce, the others wait for a file that carries it; rank 0 removes the file once the communicator exists); --exchange=ipc moves the
// partial frames on the copy engines instead of through RCCL (trhip_ipc_*: the set-up blobs travel through <file>.ipc<rank>); every rank renders its share
// of each frame, the partial frames meet on rank 0 through trhip_gather_partials, rank 0 stitches, tonemaps and saves.  With
// --shard=views the ranks divide the viewports of a camera grid instead (viewport v on rank v mod N) and save their own views.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <sstream>

#include "tauray_hip.hh"
#include "tauray_hip_comm.hh"
#include "tauray_envmap.hh"
#include "tauray_gltf.hh"

using namespace tr;

static bool starts(const std::string& s, const std::string& p) { return s.compare(0, p.size(), p) == 0; }

static const char* const usage_text =
    "usage: tauray_hip scene.glb|scene.gltf|scene.trsc [options]\n"
    "  --width=W --height=H --headless=PREFIX --frames=N --warmup-frames=N --filetype=exr|raw|none --format=rgb16|rgb32|rgba16|rgba32\n"
    "  --renderer=sh-probes --samples-per-probe=N --sh-order=0..4 --dshgi-temporal-ratio=r   bakes the scene's light-probe grids (TR_data.light_probe)\n"
    "                         as spherical harmonics; --headless=PREFIX writes PREFIX_grid<k> per grid and frame: the RGBA32F volume unfolded to\n"
    "                         width rx and height ry * (order + 1)^2 * rz, as rgba32 unless --format says otherwise (alpha is the projected\n"
    "                         distance; rgb16 / rgb32 drop it) (one device; no denoiser, --taa or reprojection)\n"
    "  --renderer=dshgi [--use-probe-visibility] [--brdf-integration=FILE.exr] --samples-per-probe=N --sh-order=0..4 --dshgi-temporal-ratio=r\n"
    "                         direct light plus indirect light looked up in the scene's light-probe grids, which are baked every frame as\n"
    "                         --renderer=sh-probes bakes them; no bounce rays per pixel.  --use-probe-visibility weighs the probes by their\n"
    "                         stored distances instead of filtering trilinearly; the BRDF-integration table is generated unless a file is named\n"
    "                         (one device; works with --animation, --headless, --camera-grid, --tonemap, --samples-per-pixel and --envmap; no\n"
    "                         denoiser, --taa, reprojection or --display=looking-glass)\n"
    "  --renderer=restir-di [--restir=candidates,spatial_samples,search_radius,max_confidence,temporal_reuse]   (4,2,32,16,on; positional or name=value)\n"
    "                         ReSTIR DI: direct light by reservoir resampling - `candidates` (1..32) light samples per pixel, one kept; the previous\n"
    "                         frame's reservoir is reused through screen motion and up to `spatial_samples` (0..4) neighbours within search_radius\n"
    "                         pixels are merged; one pass per frame (one device; works with --animation, --headless, --camera-grid, --tonemap,\n"
    "                         --envmap and -t; no denoiser, --taa, reprojection, --display=looking-glass or --samples-per-pixel above 1;\n"
    "                         --renderer=restir, the reference's ReSTIR PT, is not built)\n"
    "  --renderer=restir-gi [--restir-gi=spatial_samples,search_radius,max_confidence,temporal_reuse]   (2,32,16,on; positional or name=value)\n"
    "                         ReSTIR GI: the direct light of --renderer=restir-di (--restir= configures it) plus one bounce of indirect light by\n"
    "                         reservoir resampling - one cosine-hemisphere ray per pixel, the radiance its hit reflects kept as the sample; the\n"
    "                         previous frame's reservoir and up to `spatial_samples` (0..4) neighbours within search_radius pixels are merged\n"
    "                         (one device; works with and refuses what --renderer=restir-di does)\n"
    "  --restir-visibility=per-target|shared|sampled   (per-target) where ReSTIR DI traces shadow rays, with --renderer=restir-di and restir-gi:\n"
    "                         per-target: inside every target function, candidates + 2 * spatial_samples + 1 rays a pixel; shared: only the\n"
    "                         chosen sample's shading, 1 ray, unbiased; sampled: also the sample the candidates chose, 2 rays, biased where\n"
    "                         visibility differs between the pixels that share a sample\n"
    "  --restir-light-selection=uniform|power[,fraction]   (uniform) how ReSTIR DI draws a point or triangle light candidate, with\n"
    "                         --renderer=restir-di and restir-gi: uniform: every light of its class alike; power: in proportion to the\n"
    "                         lights' power through an alias table, the share `fraction` (0.1, in (0, 1]) of the pdf kept uniform\n"
    "  --restir-bsdf-candidates=N   (0) candidates a pixel of ReSTIR DI draws from its surface's BSDF behind the light candidates, 0..8 and at\n"
    "                         most 32 together, with --renderer=restir-di and restir-gi: each traces one closest-hit ray and takes the emissive\n"
    "                         triangle or the environment it finds; all candidates are weighted by the balance heuristic over the two techniques\n"
    "  --restir-sphere-lights=point|area   (point) how ReSTIR DI lights a point light that has a radius, with --renderer=restir-di and\n"
    "                         restir-gi: point: as a point, hard shadows; area: by samples on the sphere, soft shadows as --renderer=direct draws them\n"
    "  --restir-gi-bounces=N  the vertices of a ReSTIR GI sample's path behind the pixel, 1..8 (1): above 1 the radiance of a sample is that of a\n"
    "                         path continued from the ray's hit by cosine-hemisphere bounces with one light sample at each vertex, no\n"
    "                         Russian roulette (--max-ray-depth is not read by this renderer)\n"
    "  --renderer=path-tracer|direct --max-ray-depth=N --samples-per-pixel=N --sampler=uniform-random|sobol-owen|sobol-z2|sobol-z3 --rng-seed=N\n"
    "  --denoiser=none|bmfr   bmfr: blockwise multi-order feature regression between the path tracer and the tonemap stage\n"
    "                         (one device or --shard=views; works with --animation and --headless; svgf is not built)\n"
    "  --spatial-reprojection=i,j,...   sparse light field: only the listed viewports of --camera-grid are path traced, the others are\n"
    "                         filled from them through the G-buffer (one file per view, in natural view order; one device, no denoiser)\n"
    "  --temporal-reprojection=r        blend the previous frame, found through screen motion, into the path-traced views: r in (0, 1)\n"
    "  --taa=N[,edge-dilation=on|off][,anti-shimmer=on|off]   temporal antialiasing behind the tonemap stage: the cameras step through a\n"
    "                         jitter sequence of N sub-pixel offsets, every frame is blended into a history with weight 1 / N (edge\n"
    "                         dilation on, anti-shimmer off by default; one device; works with --animation, --headless, --denoiser=bmfr)\n"
    "  --display=headless|looking-glass   looking-glass: the cameras become the rig of a Looking Glass display under the scene's first camera and\n"
    "                         the views are interleaved, sub-pixel by sub-pixel, into the one image the lenticular panel shows: --width / --height\n"
    "                         are the size of one view, --headless=PREFIX writes one composed screenW x screenH file per frame (one device; works\n"
    "                         with --spatial-reprojection, --temporal-reprojection, --denoiser=bmfr, --taa and --animation)\n"
    "  --lkg-params=viewports,midplane,depth,relative_dist   the rig (48,2,2,2); positional or name=value\n"
    "  --lkg-calibration=display_index,pitch,slope,center,fringe,viewCone,invView,verticalAngle,DPI,screenW,screenH,flipImageX,flipImageY,flipSubp\n"
    "                         the panel, as its calibration file has it (required: no display service is read here); positional or name=value\n"
    "  --tonemap=filmic|linear|gamma-correction|reinhard|reinhard-luminance --exposure=E --gamma=G\n"
    "  --animation[=NAME] --framerate=F --accumulation --envmap=FILE --camera-grid=w,h,x,y -t --skip-nan-check\n"
    "  --deformation-motion   screen motion (--denoiser=bmfr, --taa, --temporal-reprojection, the temporal reuse of --renderer=restir-di) follows\n"
    "                         skinned and morphed meshes as they deform: their positions are kept every frame before --animation poses them\n"
    "                         (off: their rigid motion only; every renderer that plays --animation; nothing changes without a deforming mesh)\n"
    "  --fake-devices=N | --devices=0,1,... --distribution-strategy=scanline|shuffled-strips --frames-in-flight=N --frames-per-launch=N\n"
    "  --process-count=N --process-rank=R --device=D --comm-id=FILE [--comm-nonce=N] [--exchange=rccl|ipc] [--shard=views]\n"
    "  --dump-scene=out.trsc\n";

int main(int argc, char** argv)
{
    // hardware queues of the HIP runtime (default 4): more than three frame slots only pay off with more; read when the
    // runtime starts, i.e. before the first call into libtrhip
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    // memory shared between processes (RCCL, the copy-engine exchange): dmabuf IPC is what the target boxes' host driver supports
    setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
    try
    {
        std::string scene_path, prefix = "capture";
        uvec2 size{1280, 720};
        int frames = 1, warmup = 0, fake_devices = 1, frames_in_flight = 1, frames_per_launch = 1;
        std::string renderer = "path-tracer";
        int samples_per_probe = 512, sh_order = 2;                          // --samples-per-probe, --sh-order, --dshgi-temporal-ratio (src/options.hh:254-284)
        float dshgi_temporal_ratio = 0.01f;
        bool use_probe_visibility = false;                                  // --use-probe-visibility, --brdf-integration (src/options.hh, data/brdf_integration.exr)
        std::string brdf_integration_path;
        restir_di_stage::options restir;                                    // --restir
        bool restir_given = false, restir_visibility_given = false;         // --restir-visibility
        bool restir_light_selection_given = false;                          // --restir-light-selection
        bool restir_bsdf_candidates_given = false;                          // --restir-bsdf-candidates
        bool restir_sphere_lights_given = false;                            // --restir-sphere-lights
        restir_gi_stage::options restir_gi;                                 // --restir-gi
        bool restir_gi_given = false, restir_gi_bounces_given = false;       // --restir-gi-bounces
        std::vector<int> devices;
        bool timing = false;
        std::string dump_scene;
        std::string envmap_path;
        bool format_given = false;                                          // --format: sh-probes defaults to rgba32 (the alpha channel is the distance)
        bool frames_given = false, animation_flag = false;      // --animation[=name] --framerate=F (src/options.hh:110-129)
        std::string animation_name;
        double framerate = 60.0;
        int grid_w = 1, grid_h = 1;                                         // --camera-grid=w,h,x,y (src/options.hh camera_grid; generate_cameras)
        double grid_dx = 0, grid_dy = 0, grid_recentering = 5.0, grid_roll = 0;
        bool shard_views = false;                                           // --shard=views with --process-count: viewport v on rank v mod N
        int process_rank = -1, process_count = 0, process_device = 0;      // one process per GPU (see above)
        std::string comm_id_path;
        uint64_t comm_nonce = 0;
        std::string exchange = "rccl";
        std::vector<double> workloads;      // --device-workloads=a,b,...: rt_renderer::set_device_workloads before the first frame
        std::string display = "headless";                                   // --display (src/options.hh:331-341)
        uint32_t lkg_viewports = 48;                                        // --lkg-params (src/options.hh:375-385)
        double lkg_midplane = 2.0, lkg_depth = 2.0, lkg_relative_dist = 2.0;
        std::optional<looking_glass_calibration> lkg_calibration;           // --lkg-calibration (src/options.hh:386-405)
        rt_renderer::options opt;
        opt.distribution.strategy = DISTRIBUTION_SHUFFLED_STRIPS;      // CLI default (src/options.hh:43-49)
        headless::options hopt;
        hopt.single_frame = true;
        for(int i = 1; i < argc; ++i)
        {
            std::string a = argv[i];
            auto val = [&](const char* key) { return a.substr(std::strlen(key)); };
            if(a == "-t") timing = true;
            else if(a == "--help" || a == "-h") { std::cout << usage_text; return 0; }
            else if(starts(a, "--denoiser="))
            {   // --denoiser (src/options.hh; src/tauray.cc:516-517): the post-processing chain between path tracer and tonemap
                const std::string v = val("--denoiser=");
                if(v == "bmfr") opt.bmfr = bmfr_stage::options{};
                else if(v == "none") opt.bmfr.reset();
                else if(v == "svgf") throw std::runtime_error("--denoiser=svgf: the SVGF denoiser is not built (--denoiser=none|bmfr)");
                else throw std::runtime_error("--denoiser is none or bmfr, not " + v);
            }
            else if(starts(a, "--spatial-reprojection="))
            {   // --spatial-reprojection (src/options.hh; src/tauray.cc:301-305): the active viewports
                std::stringstream ss(val("--spatial-reprojection=")); std::string tok;
                while(std::getline(ss, tok, ','))
                {
                    if(tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos) throw std::runtime_error("--spatial-reprojection=i,j,...: viewport indices, not " + tok);
                    opt.spatial_reprojection.push_back((uint32_t)std::stoul(tok));
                }
                if(opt.spatial_reprojection.empty()) throw std::runtime_error("--spatial-reprojection=i,j,...: the viewport list is empty");
            }
            else if(starts(a, "--temporal-reprojection="))
            {
                opt.temporal_reprojection = std::stof(val("--temporal-reprojection="));
                if(!(opt.temporal_reprojection >= 0.0f) || !(opt.temporal_reprojection < 1.0f)) throw std::runtime_error("--temporal-reprojection=r: the ratio must be in [0, 1) (0 = off)");
            }
            else if(starts(a, "--taa="))
            {   // --taa (src/options.hh:406-411): sequence_length, edge_dilation = true, anti_shimmer = false
                std::stringstream ss(val("--taa=")); std::string tok;
                rt_renderer::options::taa_options t;
                bool first = true;
                auto on_off = [&](const std::string& v) { if(v == "on" || v == "true" || v == "1") return true; if(v == "off" || v == "false" || v == "0") return false;
                                                          throw std::runtime_error("--taa: " + v + " is neither on nor off"); };
                while(std::getline(ss, tok, ','))
                {
                    if(first)
                    {
                        if(tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos || std::stoul(tok) < 1) throw std::runtime_error("--taa=N: the length of the jitter sequence, not " + tok);
                        t.sequence_length = (int)std::stoul(tok);
                        first = false;
                    }
                    else if(starts(tok, "edge-dilation=")) t.edge_dilation = on_off(tok.substr(14));
                    else if(starts(tok, "anti-shimmer=")) t.anti_shimmer = on_off(tok.substr(13));
                    else throw std::runtime_error("--taa=N[,edge-dilation=on|off][,anti-shimmer=on|off], not " + tok);
                }
                if(first) throw std::runtime_error("--taa=N: the length of the jitter sequence is missing");
                opt.taa = t;
            }
            else if(starts(a, "--display="))
            {
                display = val("--display=");
                if(display == "window" || display == "openxr" || display == "frame-server" || display == "frame-client")
                    throw std::runtime_error("--display=" + display + ": not built (--display=headless|looking-glass)");
                if(display != "headless" && display != "looking-glass") throw std::runtime_error("--display is headless or looking-glass, not " + display);
            }
            else if(starts(a, "--lkg-params="))
            {
                const auto v = parse_struct_option("--lkg-params", val("--lkg-params="), {"viewports", "midplane", "depth", "relative_dist"});
                const double n = struct_number("--lkg-params", v, "viewports", 48);
                if(!(n >= 1) || n > 255 || n != std::floor(n)) throw std::runtime_error("--lkg-params: viewports must be a whole number in 1..255 (the composition stage's limit)");
                lkg_viewports = (uint32_t)n;
                lkg_midplane = struct_number("--lkg-params", v, "midplane", 2.0); lkg_depth = struct_number("--lkg-params", v, "depth", 2.0);
                lkg_relative_dist = struct_number("--lkg-params", v, "relative_dist", 2.0);
                if(!(lkg_midplane >= 0.001) || !(lkg_depth >= 0.001) || !(lkg_relative_dist >= 0.001)) throw std::runtime_error("--lkg-params: midplane, depth and relative_dist must be at least 0.001");
            }
            else if(starts(a, "--lkg-calibration="))
            {   // the fields the reference ignores (display_index, fringe, verticalAngle, the flips) are parsed and ignored
                const std::vector<std::string> names = {"display_index", "pitch", "slope", "center", "fringe", "viewCone", "invView", "verticalAngle", "DPI", "screenW", "screenH",
                                                        "flipImageX", "flipImageY", "flipSubp"};
                const auto v = parse_struct_option("--lkg-calibration", val("--lkg-calibration="), names);
                for(const std::string& n: names) (void)struct_number("--lkg-calibration", v, n, 0.0);
                looking_glass_calibration c;
                auto num = [&](const char* n) { return struct_number("--lkg-calibration", v, n, 0.0); };
                c.pitch = (float)num("pitch"); c.slope = (float)num("slope"); c.center = (float)num("center"); c.view_cone = (float)num("viewCone");
                c.invert = num("invView") > 0.5; c.dpi = (float)num("DPI");
                if(!(num("screenW") >= 1) || !(num("screenH") >= 1) || num("screenW") > 16384 || num("screenH") > 16384) throw std::runtime_error("--lkg-calibration: screenW and screenH must be in 1..16384");
                c.screen_w = (uint32_t)num("screenW"); c.screen_h = (uint32_t)num("screenH");
                c.check();
                lkg_calibration = c;
            }
            else if(a == "--skip-nan-check") hopt.skip_nan_check = true;     // headless::options::skip_nan_check (src/headless.hh:74); with --filetype=none: no readback at all
            else if(a == "--accumulation") opt.accumulate = true;
            else if(a == "--pre-transform-vertices") opt.pre_transformed_vertices = true;
            else if(starts(a, "--width=")) size.x = (uint32_t)std::stoul(val("--width="));
            else if(starts(a, "--height=")) size.y = (uint32_t)std::stoul(val("--height="));
            else if(starts(a, "--headless=")) prefix = val("--headless=");
            else if(starts(a, "--max-ray-depth=")) opt.max_ray_depth = std::stoi(val("--max-ray-depth="));
            else if(starts(a, "--min-ray-dist=")) opt.min_ray_dist = std::stof(val("--min-ray-dist="));
            else if(starts(a, "--samples-per-pixel=")) opt.samples_per_pixel = std::stoi(val("--samples-per-pixel="));
            else if(starts(a, "--samples-per-pass=")) opt.samples_per_pass = std::stoi(val("--samples-per-pass="));
            else if(starts(a, "--frames=")) { frames = std::stoi(val("--frames=")); hopt.single_frame = frames == 1; frames_given = true; }
            else if(a == "--animation") animation_flag = true;                                  // any clip a node has (src/tauray.cc:252-253)
            else if(starts(a, "--animation=")) { animation_flag = true; animation_name = val("--animation="); }
            else if(starts(a, "--framerate=")) framerate = std::stod(val("--framerate="));
            else if(a == "--deformation-motion") opt.scene.deformation_motion = true;             // scene_stage::options (trhip_scene_set_deformation_motion)
            else if(starts(a, "--envmap=")) envmap_path = val("--envmap=");                        // lat-long .hdr (src/options.hh:125)
            else if(starts(a, "--warmup-frames=")) warmup = std::stoi(val("--warmup-frames="));
            else if(starts(a, "--renderer="))
            {
                renderer = val("--renderer=");
                if(renderer != "path-tracer" && renderer != "direct" && renderer != "sh-probes" && renderer != "dshgi" && renderer != "restir-di" && renderer != "restir-gi")
                    throw std::runtime_error("unknown renderer " + renderer + " (path-tracer, direct, sh-probes, dshgi, restir-di, restir-gi)");
            }
            else if(starts(a, "--restir=")) { restir.parse(val("--restir=")); restir_given = true; }
            else if(starts(a, "--restir-visibility=")) { restir.parse_visibility(val("--restir-visibility=")); restir_visibility_given = true; }
            else if(starts(a, "--restir-light-selection=")) { restir.parse_light_selection(val("--restir-light-selection=")); restir_light_selection_given = true; }
            else if(starts(a, "--restir-bsdf-candidates=")) { restir.parse_bsdf_candidates(val("--restir-bsdf-candidates=")); restir_bsdf_candidates_given = true; }
            else if(starts(a, "--restir-sphere-lights=")) { restir.parse_sphere_lights(val("--restir-sphere-lights=")); restir_sphere_lights_given = true; }
            else if(starts(a, "--restir-gi=")) { restir_gi.parse(val("--restir-gi=")); restir_gi_given = true; }
            else if(starts(a, "--restir-gi-bounces=")) { restir_gi.parse_bounces(val("--restir-gi-bounces=")); restir_gi_bounces_given = true; }
            else if(a == "--use-probe-visibility") use_probe_visibility = true;
            else if(starts(a, "--brdf-integration=")) brdf_integration_path = val("--brdf-integration=");
            else if(starts(a, "--samples-per-probe="))
            {   // src/options.hh:254-257
                samples_per_probe = std::stoi(val("--samples-per-probe="));
                if(samples_per_probe < 1) throw std::runtime_error("--samples-per-probe=N: at least one sample per probe, not " + val("--samples-per-probe="));
            }
            else if(starts(a, "--sh-order="))
            {   // src/options.hh:282-284
                sh_order = std::stoi(val("--sh-order="));
                if(sh_order < 0 || sh_order > 4) throw std::runtime_error("--sh-order=O: the order is 0 ... 4, not " + val("--sh-order="));
            }
            else if(starts(a, "--dshgi-temporal-ratio="))
            {   // src/options.hh:258-260
                dshgi_temporal_ratio = std::stof(val("--dshgi-temporal-ratio="));
                if(!(dshgi_temporal_ratio >= 0.0f) || !(dshgi_temporal_ratio <= 1.0f)) throw std::runtime_error("--dshgi-temporal-ratio=r: the ratio is in [0, 1]");
            }
            else if(starts(a, "--dump-scene=")) dump_scene = val("--dump-scene=");
            else if(starts(a, "--as-strategy="))     // scene_stage::options::group_strategy (src/options.hh:519-532); see trhip.h
            {
                const std::string v = val("--as-strategy=");
                if(v == "all-merged") opt.scene.as_strategy = TRHIP_AS_ALL_MERGED;
                else if(v == "per-material" || v == "per-model") opt.scene.as_strategy = TRHIP_AS_PER_MESH;   // an instance is one primitive
                else if(v == "static-merged-dynamic-per-model") opt.scene.as_strategy = TRHIP_AS_STATIC_MERGED_DYNAMIC_PER_MESH;
                else throw std::runtime_error("unknown --as-strategy=" + v + " (all-merged, per-material, per-model, static-merged-dynamic-per-model)");
            }
            else if(starts(a, "--device-workloads="))
            {
                std::string v = val("--device-workloads=");
                for(size_t p0 = 0; p0 <= v.size();)
                {
                    size_t p1 = v.find(',', p0);
                    if(p1 == std::string::npos) p1 = v.size();
                    workloads.push_back(std::stod(v.substr(p0, p1 - p0)));
                    p0 = p1 + 1;
                }
            }
            else if(starts(a, "--frames-in-flight=")) frames_in_flight = std::max(1, std::stoi(val("--frames-in-flight=")));
            else if(starts(a, "--frames-per-launch=")) frames_per_launch = std::max(1, std::stoi(val("--frames-per-launch=")));   // rt_renderer::options::frames_per_launch
            else if(starts(a, "--camera-grid="))
            {
                std::stringstream ss(val("--camera-grid=")); std::string tok; std::vector<double> v;
                while(std::getline(ss, tok, ',')) v.push_back(std::stod(tok));
                if(v.size() != 4 || v[0] < 1 || v[1] < 1) throw std::runtime_error("--camera-grid=w,h,x,y");
                grid_w = (int)v[0]; grid_h = (int)v[1]; grid_dx = v[2]; grid_dy = v[3];
            }
            else if(starts(a, "--camera-recentering-distance=")) grid_recentering = std::stod(val("--camera-recentering-distance="));
            else if(starts(a, "--camera-grid-roll=")) grid_roll = std::stod(val("--camera-grid-roll="));
            else if(starts(a, "--shard="))
            {
                const std::string v = val("--shard=");
                if(v != "views" && v != "pixels") throw std::runtime_error("--shard=pixels|views");
                shard_views = v == "views";
            }
            else if(starts(a, "--process-rank=")) process_rank = std::stoi(val("--process-rank="));
            else if(starts(a, "--process-count=")) process_count = std::stoi(val("--process-count="));
            else if(starts(a, "--device=")) process_device = std::stoi(val("--device="));
            else if(starts(a, "--comm-id=")) comm_id_path = val("--comm-id=");
            else if(starts(a, "--comm-nonce=")) comm_nonce = std::stoull(val("--comm-nonce="));
            else if(starts(a, "--exchange=")) exchange = val("--exchange=");
            else if(starts(a, "--fake-devices=")) fake_devices = std::stoi(val("--fake-devices="));
            else if(starts(a, "--rng-seed=")) opt.rng_seed = std::stoi(val("--rng-seed="));
            else if(starts(a, "--exposure=")) opt.tonemap.exposure = std::stof(val("--exposure="));
            else if(starts(a, "--gamma=")) opt.tonemap.gamma = std::stof(val("--gamma="));
            else if(starts(a, "--devices="))
            {
                std::stringstream ss(val("--devices=")); std::string tok;
                while(std::getline(ss, tok, ',')) devices.push_back(std::stoi(tok));
            }
            else if(starts(a, "--distribution-strategy="))
            {
                std::string v = val("--distribution-strategy=");
                opt.distribution.strategy = v == "scanline" ? DISTRIBUTION_SCANLINE : v == "duplicate" ? DISTRIBUTION_DUPLICATE : DISTRIBUTION_SHUFFLED_STRIPS;
            }
            else if(starts(a, "--filetype="))
            {
                std::string v = val("--filetype=");
                hopt.output_file_type = v == "raw" ? headless::RAW : (v == "none" ? headless::EMPTY : headless::EXR);
            }
            else if(starts(a, "--compression="))
            {
                static const std::map<std::string, tr::headless::compression_type> comps = {
                    {"none", tr::headless::NONE}, {"rle", tr::headless::RLE}, {"zips", tr::headless::ZIPS}, {"zip", tr::headless::ZIP}, {"piz", tr::headless::PIZ}};
                auto it = comps.find(val("--compression="));
                if(it == comps.end()) throw std::runtime_error("unknown compression " + val("--compression="));
                hopt.output_compression = it->second;
            }
            else if(starts(a, "--format="))
            {
                std::string v = val("--format=");
                format_given = true;
                hopt.output_format = v == "rgb32" ? headless::RGB32 : v == "rgba16" ? headless::RGBA16 : v == "rgba32" ? headless::RGBA32 : headless::RGB16;
            }
            else if(starts(a, "--tonemap="))
            {
                static const std::map<std::string, tonemap_stage::operator_type> ops = {
                    {"linear", tonemap_stage::LINEAR}, {"gamma-correction", tonemap_stage::GAMMA_CORRECTION}, {"filmic", tonemap_stage::FILMIC},
                    {"reinhard", tonemap_stage::REINHARD}, {"reinhard-luminance", tonemap_stage::REINHARD_LUMINANCE}};
                auto it = ops.find(val("--tonemap="));
                if(it == ops.end()) throw std::runtime_error("unknown tonemap operator");
                opt.tonemap.tonemap_operator = it->second;
            }
            else if(starts(a, "--sampler="))
            {
                std::string v = val("--sampler=");
                opt.local_sampler = v == "sobol-owen" ? sampler_type::SOBOL_OWEN : v == "sobol-z2" ? sampler_type::SOBOL_Z_ORDER_2D :
                    v == "sobol-z3" ? sampler_type::SOBOL_Z_ORDER_3D : sampler_type::UNIFORM_RANDOM;
            }
            else if(starts(a, "--")) throw std::runtime_error("unknown option " + a);
            else scene_path = a;
        }
        if(scene_path.empty()) throw std::runtime_error(usage_text);
        if(renderer == "dshgi" && display == "looking-glass") throw std::runtime_error("--renderer=dshgi: no --display=looking-glass (the composition of a light field from it is not built)");
        if(restir_given && renderer != "restir-di" && renderer != "restir-gi") throw std::runtime_error("--restir sets the options of --renderer=restir-di");
        if(restir_visibility_given && renderer != "restir-di" && renderer != "restir-gi")
            throw std::runtime_error("--restir-visibility sets the visibility mode of --renderer=restir-di");
        if(restir_light_selection_given && renderer != "restir-di" && renderer != "restir-gi")
            throw std::runtime_error("--restir-light-selection sets the light selection of --renderer=restir-di");
        if(restir_bsdf_candidates_given && renderer != "restir-di" && renderer != "restir-gi")
            throw std::runtime_error("--restir-bsdf-candidates sets the BSDF candidates of --renderer=restir-di");
        if(restir_sphere_lights_given && renderer != "restir-di" && renderer != "restir-gi")
            throw std::runtime_error("--restir-sphere-lights sets how --renderer=restir-di lights a point light that has a radius");
        if(restir_bsdf_candidates_given) restir.check();      // the two counts together, said before a scene is read
        if(restir_gi_given && renderer != "restir-gi") throw std::runtime_error("--restir-gi sets the options of --renderer=restir-gi");
        if(restir_gi_bounces_given && renderer != "restir-gi") throw std::runtime_error("--restir-gi-bounces sets the path length of --renderer=restir-gi");
        if(renderer == "restir-gi")
        {   // what the renderer does not do, said before a scene is read
            if(opt.bmfr) throw std::runtime_error("--renderer=restir-gi: no --denoiser (the resampling is the noise reduction; the denoiser's feature targets are not written)");
            if(opt.taa) throw std::runtime_error("--renderer=restir-gi: no --taa (the stages write no screen_motion target and their cameras do not jitter)");
            if(!opt.spatial_reprojection.empty() || opt.temporal_reprojection > 0.0f)
                throw std::runtime_error("--renderer=restir-gi: no --spatial-reprojection or --temporal-reprojection (the stages write no G-buffer targets)");
            if(display == "looking-glass") throw std::runtime_error("--renderer=restir-gi: no --display=looking-glass (the composition of a light field from it is not built)");
            if(opt.samples_per_pixel > 1) throw std::runtime_error("--renderer=restir-gi: one pass per frame, --samples-per-pixel must be 1 (the reservoirs carry the samples from frame to frame)");
            if(devices.size() > 1 || fake_devices > 1) throw std::runtime_error("--renderer=restir-gi runs on one device: the reservoirs of neighbouring pixels and of the previous frame live on one device");
            if(process_count > 0 || shard_views) throw std::runtime_error("--renderer=restir-gi runs in one process: no --process-count or --shard");
        }
        if(renderer == "restir-di")
        {   // what the renderer does not do, said before a scene is read
            if(opt.bmfr) throw std::runtime_error("--renderer=restir-di: no --denoiser (the resampling is the noise reduction; the denoiser's feature targets are not written)");
            if(opt.taa) throw std::runtime_error("--renderer=restir-di: no --taa (the stage writes no screen_motion target and its cameras do not jitter)");
            if(!opt.spatial_reprojection.empty() || opt.temporal_reprojection > 0.0f)
                throw std::runtime_error("--renderer=restir-di: no --spatial-reprojection or --temporal-reprojection (the stage writes no G-buffer targets)");
            if(display == "looking-glass") throw std::runtime_error("--renderer=restir-di: no --display=looking-glass (the composition of a light field from it is not built)");
            if(opt.samples_per_pixel > 1) throw std::runtime_error("--renderer=restir-di: one pass per frame, --samples-per-pixel must be 1 (raise the candidates of --restir instead)");
            if(devices.size() > 1 || fake_devices > 1) throw std::runtime_error("--renderer=restir-di runs on one device: the reservoirs of neighbouring pixels and of the previous frame live on one device");
            if(process_count > 0 || shard_views) throw std::runtime_error("--renderer=restir-di runs in one process: no --process-count or --shard");
        }
        if(devices.empty()) devices.assign((size_t)std::max(fake_devices, 1), 0);

        const bool is_glb = (scene_path.size() > 4 && scene_path.compare(scene_path.size() - 4, 4, ".glb") == 0) ||
                            (scene_path.size() > 5 && scene_path.compare(scene_path.size() - 5, 5, ".gltf") == 0);
        scene_data scene = is_glb ? load_glb(scene_path, size.x, size.y) : load_scene_dump(scene_path);
        if(!envmap_path.empty()) set_envmap(scene, envmap_path);      // src/tauray.cc:198-201
        uint32_t viewports = 1;
        const bool looking_glass = display == "looking-glass";
        if(looking_glass)
        {   // looking_glass::setup_cameras with the metadata of --lkg-calibration (src/looking_glass.cc:62-88, 216-242)
            if(!lkg_calibration)
                throw std::runtime_error("--display=looking-glass needs --lkg-calibration=...: no display service is read here (the reference asks the HoloPlay service "
                                         "of the machine the display hangs on; give the panel's calibration file on the command line instead)");
            if(grid_w * grid_h > 1) throw std::runtime_error("--display=looking-glass sets the cameras up itself: no --camera-grid");
            if(!is_glb) throw std::runtime_error("--display=looking-glass hangs its rig on the first camera of a glTF scene");
            if(devices.size() > 1 || process_count > 0 || shard_views)
                throw std::runtime_error("--display=looking-glass with several devices or processes: the composition stage reads every view of the light field on one device, "
                                         "the views would have to be gathered first, which is not built; use one device");
            if(frames_per_launch > 1) throw std::runtime_error("--display=looking-glass: a composed frame is one frame, --frames-per-launch must be 1");
            viewports = looking_glass_cameras(scene, lkg_viewports, lkg_midplane, lkg_depth, lkg_relative_dist, *lkg_calibration);
            rt_renderer::options::looking_glass_options lo;
            lo.stage.viewport_count = viewports; lo.stage.pitch = lkg_calibration->corrected_pitch(); lo.stage.tilt = lkg_calibration->tilt();
            lo.stage.center = lkg_calibration->center; lo.stage.invert = lkg_calibration->invert;
            lo.output_size = uvec2{lkg_calibration->screen_w, lkg_calibration->screen_h};
            opt.looking_glass = lo;
        }
        if(grid_w * grid_h > 1) viewports = generate_cameras(scene, grid_w, grid_h, grid_dx, grid_dy, grid_recentering, grid_roll);      // src/tauray.cc:680-727
        // play(scene, name, !replay, name == "") (src/tauray.cc:252-253); ticks in microseconds per update (:1052)
        scene_animator animator(scene);
        if(animation_flag) animator.play(animation_name, false);
        const int64_t update_dt = (int64_t)std::floor(1000000.0 / framerate + 0.5);
        const bool animated = animation_flag && animator.is_playing();
        if(animated && scene.animation)
        {   // the instances placed by an animated node or one below it are dynamic (!static_transformable)
            opt.scene.dynamic.assign(scene.instance_count(), 0);
            std::vector<int> todo;
            for(const auto& c: scene.animation->clips) todo.push_back(c.first);
            while(!todo.empty())
            {
                const int n = todo.back(); todo.pop_back();
                auto it = scene.animation->nodes.find(n);
                if(it == scene.animation->nodes.end()) continue;
                for(uint32_t i: it->second.instances) if(i < opt.scene.dynamic.size()) opt.scene.dynamic[i] = 1;
                for(int c: it->second.children) todo.push_back(c);
            }
        }
        if(animated && !frames_given) { frames = std::numeric_limits<int>::max(); hopt.single_frame = false; }      // until the clip ends
        if(!dump_scene.empty())
        {
            // with --animation the dump is the scene after --frames updates (the first one by dt = 0)
            if(animated) for(int f = 0; f < (frames_given ? frames : 1); ++f) animator.update(f == 0 ? 0 : update_dt);   // the flattened scene, and next to it what the loader found of skins: per skinned instance u32 instance, u32 vertices,
            // u32 joints, the {joints, weights} records, the rest-pose joint matrices
            write_scene_dump(scene, dump_scene);
            if(!scene.skinned.empty())
            {
                std::ofstream f(dump_scene + ".skins", std::ios::binary);
                for(const auto& sk: scene.skinned)
                {
                    const uint32_t head[3] = {sk.instance, (uint32_t)sk.skins.size(), (uint32_t)(sk.joint_transforms.size() / 16)};
                    f.write(reinterpret_cast<const char*>(head), 12);
                    f.write(reinterpret_cast<const char*>(sk.skins.data()), (std::streamsize)(sk.skins.size() * sizeof(trhip_skin)));
                    f.write(reinterpret_cast<const char*>(sk.joint_transforms.data()), (std::streamsize)(sk.joint_transforms.size() * 4));
                }
            }
            return 0;
        }
        // create_renderer (src/tauray.cc:355-421): classes without lights get weight 0, projection follows the camera
        if(scene.point_light_count() == 0) opt.sampling_weights.point_lights = 0;
        if(scene.directional_light_count() == 0) opt.sampling_weights.directional_lights = 0;
        if(scene.envmap.empty()) opt.sampling_weights.envmap = 0;
        if(!scene.has_tri_lights()) opt.sampling_weights.emissive_triangles = 0;
        opt.projection = (int)scene.projection;
        opt.samples_per_pass = std::min(opt.samples_per_pass, opt.samples_per_pixel);
        opt.active_viewport_count = viewports;

        // the bake's options (sh-probes, dshgi): the path tracer's, with the probes' sample count and history ratio
        auto sh_options = [&]
        {
            sh_renderer::options so;
            so.max_ray_depth = opt.max_ray_depth; so.min_ray_dist = opt.min_ray_dist; so.rng_seed = opt.rng_seed; so.local_sampler = opt.local_sampler;
            so.samples_per_probe = samples_per_probe; so.film = opt.film; so.film_radius = opt.film_radius; so.mis_mode = opt.mis_mode;
            so.russian_roulette_delta = opt.russian_roulette_delta; so.temporal_ratio = dshgi_temporal_ratio; so.indirect_clamping = opt.indirect_clamping;
            so.regularization_gamma = opt.regularization_gamma; so.sampling_weights = opt.sampling_weights;
            so.bounce_mode = opt.bounce_mode; so.tri_light_mode = opt.tri_light_mode;
            return so;
        };
        // The frames of a renderer of whole viewports on one device (dshgi, restir-di, restir-gi): make(dev, ss) builds it on the uploaded scene,
        // scene_moved(r) runs after an animation step has been applied, print_timings(r) prints the lines of a frame under "DEVICE 0".
        auto run_viewport_frames = [&](auto make, auto scene_moved, auto print_timings)
        {
            hopt.size = size; hopt.output_prefix = prefix; hopt.display_count = viewports;
            headless out(hopt);
            device dev(devices[0]);
            scene_stage ss(dev, opt.scene);
            ss.set_scene(scene);
            auto r = make(dev, ss);
            for(int f = -warmup; f < frames; ++f)
            {
                if(animated && f >= 0)
                {   // update(s, dt, true) before the frame, the first one by dt = 0 (src/tauray.cc:1064-1092)
                    if(!frames_given && !animator.is_playing()) break;
                    animator.update(f == 0 ? 0 : update_dt);
                    if(!frames_given && !animator.is_playing()) break;
                    dev.sync();
                    ss.apply(scene, f % 3 == 2);
                    scene_moved(*r);
                }
                r->render();
                dev.sync();
                if(f < 0) continue;
                if(timing)
                {
                    std::cout << "FRAME " << f << ":\n\tDEVICE 0:\n";
                    print_timings(*r);
                }
                out.save(dev, r->display, (unsigned)f);
            }
        };
        if(renderer == "sh-probes")
        {   // sh_renderer (src/tauray.cc:423-433, src/sh_renderer.cc): bakes the scene's probe grids, one sh_path_tracer_stage per grid
            if(opt.bmfr || opt.taa || !opt.spatial_reprojection.empty() || opt.temporal_reprojection > 0.0f)
                throw std::runtime_error("--renderer=sh-probes bakes probe grids: a denoiser, --taa and reprojection do not apply");
            if(devices.size() > 1 || process_count > 0 || shard_views)
                throw std::runtime_error("--renderer=sh-probes runs on one device: the probes of a grid share one history on one device, baking across several is not built");
            if(looking_glass || grid_w * grid_h > 1) throw std::runtime_error("--renderer=sh-probes renders no camera: no --display=looking-glass, no --camera-grid");
            if(opt.local_sampler != sampler_type::UNIFORM_RANDOM)
                throw std::runtime_error("--renderer=sh-probes: --sampler must be uniform-random (the Sobol samplers take their index from a pixel launch)");
            if(scene.sh_grids.empty())
                throw std::runtime_error("--renderer=sh-probes: " + scene_path + " has no light-probe grid (a node with TR_data.light_probe of type GRID)");
            for(sh_grid& g: scene.sh_grids) g.order = sh_order;      // src/tauray.cc:151
            const sh_renderer::options so = sh_options();
            device dev(devices[0]);
            scene_stage ss(dev, opt.scene);
            ss.set_scene(scene);
            sh_renderer sr(dev, scene.sh_grids, so);
            for(int f = -warmup; f < frames; ++f)
            {
                sr.render();
                dev.sync();
                if(f < 0) continue;
                if(timing)
                {
                    std::cout << "FRAME " << f << ":\n\tDEVICE 0:\n";
                    for(auto& st: sr.stages) { const trhip_sh_timings t = st->get_timings(); std::cout << "\t\t[" << t.name << "] " << t.total_ms << " ms\n"; }
                }
                for(size_t k = 0; k < sr.stages.size(); ++k)
                {   // the RGBA32F volume unfolded to width rx, height ry * C * rz
                    headless::options go = hopt;
                    go.size = sr.stages[k]->unfolded_size(); go.output_prefix = prefix + "_grid" + std::to_string(k); go.display_count = 1;
                    if(!format_given) go.output_format = headless::RGBA32;      // coefficients, not colours: full precision, and alpha holds the distance
                    headless gout(go);
                    const std::vector<float> img = sr.stages[k]->download();
                    gout.write_image(gout.get_filename(0, (unsigned)f), img.data());
                }
            }
            return 0;
        }
        if(renderer == "dshgi")
        {   // dshgi_renderer (src/tauray.cc:355-421, src/dshgi_renderer.cc): the grids are baked, the direct stage renders, the indirect light of the grids is added
            if(opt.bmfr || opt.taa || !opt.spatial_reprojection.empty() || opt.temporal_reprojection > 0.0f)
                throw std::runtime_error("--renderer=dshgi: a denoiser, --taa and reprojection do not apply");
            if(devices.size() > 1 || process_count > 0 || shard_views)
                throw std::runtime_error("--renderer=dshgi runs on one device: the grids' histories and the frame live on one device");
            if(opt.local_sampler != sampler_type::UNIFORM_RANDOM)
                throw std::runtime_error("--renderer=dshgi: --sampler must be uniform-random (the bake's Sobol samplers would take their index from a pixel launch)");
            if(scene.sh_grids.empty())
                throw std::runtime_error("--renderer=dshgi: " + scene_path + " has no light-probe grid (a node with TR_data.light_probe of type GRID)");
            for(sh_grid& g: scene.sh_grids) g.order = sh_order;      // src/tauray.cc:151
            dshgi_renderer::options go;
            go.direct = opt;
            go.sh = sh_options();
            go.use_probe_visibility = use_probe_visibility;
            go.tonemap = opt.tonemap;
            if(!brdf_integration_path.empty())
            {   // texture(brdf_integration, uv).xy: the file's R and G, row 0 first
                int channels = 0;
                const std::vector<float> f = exr::load_exr(brdf_integration_path, go.brdf_integration_width, go.brdf_integration_height, channels);
                if(channels < 2) throw std::runtime_error("--brdf-integration=" + brdf_integration_path + ": a BRDF-integration table has the channels R (scale) and G (bias)");
                go.brdf_integration.resize(size_t(go.brdf_integration_width) * go.brdf_integration_height * 2);
                for(size_t i = 0; i < go.brdf_integration.size() / 2; ++i) { go.brdf_integration[2 * i] = f[i * (size_t)channels]; go.brdf_integration[2 * i + 1] = f[i * (size_t)channels + 1]; }
            }
            run_viewport_frames([&](device& dev, scene_stage& ss) { return std::make_unique<dshgi_renderer>(dev, ss, scene, size, go); },
                                [&](dshgi_renderer& gr) { gr.set_scene(scene); },      // the instances pick their grids again
                                [&](dshgi_renderer& gr)
            {
                for(auto& st: gr.sh.stages) { const trhip_sh_timings t = st->get_timings(); std::cout << "\t\t[" << t.name << "] " << t.total_ms << " ms\n"; }
                std::cout << "\t\t[direct (" << viewports << " viewports)] " << gr.direct->get_duration_ms() << " ms\n";
                const trhip_dshgi_timings t = gr.indirect->get_timings();
                std::cout << "\t\t[" << t.name << "] " << t.total_ms << " ms\n";
            });
            return 0;
        }
        if(renderer == "restir-di")
        {
            restir_di_renderer::options ro;
            ro.restir = restir;
            ro.restir.min_ray_dist = opt.min_ray_dist; ro.restir.rng_seed = (uint32_t)opt.rng_seed; ro.restir.projection = opt.projection;
            ro.tonemap = opt.tonemap;
            ro.restir.check();
            run_viewport_frames([&](device& dev, scene_stage&) { return std::make_unique<restir_di_renderer>(dev, scene, size, ro); },
                                [](restir_di_renderer& rr) { rr.scene_moved(); },
                                [](restir_di_renderer& rr)
            {
                const trhip_restir_di_timings t = rr.stage->get_timings();
                std::cout << "\t\t[" << t.canonical_name << "] " << t.canonical_ms << " ms\n\t\t[" << t.spatial_name << "] " << t.spatial_ms << " ms\n";
            });
            return 0;
        }
        if(renderer == "restir-gi")
        {
            restir_gi_renderer::options ro;
            ro.restir = restir;
            ro.restir.min_ray_dist = opt.min_ray_dist; ro.restir.rng_seed = (uint32_t)opt.rng_seed; ro.restir.projection = opt.projection;
            ro.restir_gi = restir_gi;
            ro.restir_gi.min_ray_dist = opt.min_ray_dist; ro.restir_gi.rng_seed = (uint32_t)opt.rng_seed; ro.restir_gi.projection = opt.projection;
            ro.tonemap = opt.tonemap;
            ro.restir.check();
            ro.restir_gi.check();
            run_viewport_frames([&](device& dev, scene_stage&) { return std::make_unique<restir_gi_renderer>(dev, scene, size, ro); },
                                [](restir_gi_renderer& rr) { rr.scene_moved(); },
                                [](restir_gi_renderer& rr)
            {
                const trhip_restir_di_timings d = rr.direct->get_timings();
                std::cout << "\t\t[" << d.canonical_name << "] " << d.canonical_ms << " ms\n\t\t[" << d.spatial_name << "] " << d.spatial_ms << " ms\n";
                const trhip_restir_gi_timings t = rr.stage->get_timings();
                std::cout << "\t\t[" << t.initial_name << "] " << t.initial_ms << " ms\n\t\t[" << t.temporal_name << "] " << t.temporal_ms << " ms\n\t\t["
                          << t.spatial_name << "] " << t.spatial_ms << " ms\n";
            });
            return 0;
        }
        opt.max_frames_in_flight = frames_in_flight;
        opt.frames_per_launch = frames_per_launch;
        if(!opt.spatial_reprojection.empty() || opt.temporal_reprojection > 0.0f)
        {   // what rt_renderer refuses, said before a device is touched
            const std::string which = !opt.spatial_reprojection.empty() ? "--spatial-reprojection" : "--temporal-reprojection";
            if(!opt.spatial_reprojection.empty()) check_viewport_list(opt.spatial_reprojection, viewports, "--spatial-reprojection");
            if(devices.size() > 1 || process_count > 0 || shard_views)
                throw std::runtime_error(which + " with several devices or processes: the stages read the G-buffer of whole viewports on one device, "
                                         "gathering it from several is not built; use one device");
            if(opt.bmfr) throw std::runtime_error(which + " together with --denoiser=bmfr: a chain of reprojection and a denoiser is not built");
            if(frames_per_launch > 1) throw std::runtime_error(which + ": a reprojected frame is one frame, --frames-per-launch must be 1");
            if(opt.temporal_reprojection > 0.0f && opt.accumulate) throw std::runtime_error("--temporal-reprojection blends the previous frame into a fresh frame: no --accumulation");
            // a viewport that nothing reprojects to holds NaN (src/tauray.cc:301-305)
            if(!opt.spatial_reprojection.empty()) hopt.skip_nan_check = true;
        }
        if(opt.taa)
        {   // what rt_renderer refuses, said before a device is touched
            if(devices.size() > 1 || process_count > 0 || shard_views)
                throw std::runtime_error("--taa with several devices or processes: the stage reads screen motion, pos and instance id of whole viewports on one device, "
                                         "gathering them from several is not built; use one device");
            if(opt.accumulate) throw std::runtime_error("--taa blends a fresh, jittered frame into its history: no --accumulation");
            if(frames_per_launch > 1) throw std::runtime_error("--taa: an antialiased frame is one frame (the jitter steps between frames), --frames-per-launch must be 1");
            if(!opt.spatial_reprojection.empty() || opt.temporal_reprojection > 0.0f) throw std::runtime_error("--taa together with spatial / temporal reprojection: a chain of reprojection and taa is not built");
            if(opt.projection == 2) throw std::runtime_error("--taa with equirectangular cameras is not built");
            if(renderer != "path-tracer") throw std::runtime_error("--taa reads the path tracer's screen_motion target: --renderer=path-tracer");
            set_camera_jitter(scene, gltf_detail::get_camera_jitter_sequence(opt.taa->sequence_length, size.x, size.y));      // src/tauray.cc:816
        }
        hopt.size = size; hopt.output_prefix = prefix; hopt.display_count = viewports;
        if(looking_glass)
        {   // one composed frame of the panel's size per frame instead of a file per view
            if(opt.projection != 0) throw std::runtime_error("--display=looking-glass: the rig's cameras are perspective cameras");
            hopt.size = opt.looking_glass->output_size; hopt.display_count = 1;
        }
        if(shard_views)
        {   // view shards: viewport v belongs to rank v mod N; every rank renders, tonemaps and saves its own
            // views under their global indices, nothing is exchanged
            if(process_count < 1 || process_rank < 0 || process_rank >= process_count) throw std::runtime_error("--shard=views needs --process-count and --process-rank");
            if(animated || renderer != "path-tracer") throw std::runtime_error("--shard=views renders still frames with the path tracer");
            const uint32_t mine = viewports > (uint32_t)process_rank ? (viewports - (uint32_t)process_rank + (uint32_t)process_count - 1) / (uint32_t)process_count : 0;
            if(mine == 0) return 0;
            opt.active_viewport_count = mine;
            hopt.display_count = mine; hopt.display_count_total = viewports; hopt.display_index_base = (unsigned)process_rank; hopt.display_index_stride = (unsigned)process_count;
            headless vout(hopt);
            rt_renderer rr({process_device}, scene, size, opt);
            for(auto& sl: rr.per_device[0].slots) sl.ray_tracer->set_shard((uint32_t)process_rank, (uint32_t)process_count);
            for(int f = -warmup; f < frames; ++f)
            {
                rr.reset_accumulation();
                rr.render();
                rr.finish_frame();
                if(f >= 0) vout.save(*rr.per_device[0].dev, rr.display, (unsigned)f);
            }
            return 0;
        }
        headless out(hopt);
        if(process_count > 0)
        {   // one process per GPU: this process is rank process_rank of process_count
            if(process_rank < 0 || process_rank >= process_count) throw std::runtime_error("--process-rank must be in [0, --process-count)");
            if(comm_id_path.empty()) throw std::runtime_error("--process-count needs --comm-id=<file every rank can read>");
            if(renderer != "path-tracer" || animated) throw std::runtime_error("--process-count renders still frames with the path tracer");
            if(exchange != "rccl" && exchange != "ipc") throw std::runtime_error("--exchange is rccl or ipc");
            std::vector<char> id;
            if(exchange == "rccl") id = exchange_comm_id_through_file(comm_id_path, process_rank, comm_nonce);
            process_rt_renderer rr(process_device, process_rank, process_count, exchange == "rccl" ? id.data() : nullptr, scene, size, opt);
            if(exchange == "rccl") remove_comm_id_file(comm_id_path, process_rank);   // the communicator exists on every rank: the file has done its job
            else rr.use_copy_engine_exchange([&](const std::vector<char>& blob) { return allgather_blobs_through_files(comm_id_path, process_rank, process_count, blob, comm_nonce); });
            // all ranks shade with the same program, or none renders (needs the job's nonce like the blobs above; without one - a one-rank
            // job, or RCCL ranks started without --comm-nonce - there is nothing to tell this job's files from another's and the check is skipped with a note)
            if(process_count > 1 && comm_nonce != 0)
                rr.check_same_program([&](const std::vector<char>& blob) { return allgather_blobs_through_files(comm_id_path, process_rank, process_count, blob, comm_nonce, 120.0, ".prog"); });
            else if(process_count > 1 && process_rank == 0)
                std::cerr << "tauray_hip: no --comm-nonce: the ranks' shading programs are not compared (trhip_pt_get_program)\n";
            if(!workloads.empty()) rr.set_device_workloads(workloads);
            for(int f = -warmup; f < frames; ++f)
            {
                auto t0 = std::chrono::high_resolution_clock::now();
                rr.reset_accumulation();
                rr.render();
                rr.finish_frame();
                auto t1 = std::chrono::high_resolution_clock::now();
                if(f < 0) continue;
                if(timing)
                    std::cout << "FRAME " << f << ":\n\tRANK " << process_rank << ":\n\t\t[path tracing (" << opt.active_viewport_count << " viewports)] "
                              << rr.get_path_tracing_time() << " ms\n\tHOST: " << std::chrono::duration<double, std::milli>(t1 - t0).count() << " ms\n";
                if(process_rank == 0) out.save(rr.dev, rr.display, (unsigned)f);
            }
            return 0;
        }
        // --renderer picks the pipeline rt_renderer<Pipeline> is instantiated with (src/tauray.cc:355-421: path-tracer, direct)
        auto run = [&](auto& rr) -> int
        {
        if(!workloads.empty())
        {
            if(workloads.size() != rr.per_device.size()) throw std::runtime_error("--device-workloads needs one ratio per device");
            rr.set_device_workloads(workloads);
        }
        if((frames_in_flight > 1 || frames_per_launch > 1) && !animated && !opt.taa && !opt.looking_glass)
        {   // frame f renders while the frames before it are read back, compressed and written (the reference overlaps
            // its save workers with the next frames the same way, src/headless.cc:349-422); with --frames-per-launch=B a slot
            // holds B consecutive frames, frame-major in its display image
            const int B = frames_per_launch, none = std::numeric_limits<int>::min();
            const size_t frame_bytes = size_t(size.x) * size.y * 16 * opt.active_viewport_count;
            std::vector<int> in_slot(frames_in_flight, none);      // the first frame of the launch a slot holds (negative: warm-up)
            auto retire = [&](int k) {
                if(in_slot[k] == none) return;
                rr.finish_slot(k);
                for(int b = 0; b < B; ++b)
                {
                    const int f = in_slot[k] + b;
                    if(f >= 0 && f < frames)
                        out.save(*rr.per_device[0].dev, static_cast<const char*>(rr.frame_slots[k].display) + size_t(b) * frame_bytes, (unsigned)f);
                }
                in_slot[k] = none;
            };
            auto t0 = std::chrono::high_resolution_clock::now();
            bool started = false;
            for(int f = -warmup; f < frames; f += B)
            {
                const int k = (int)((rr.frame_index / (uint32_t)B) % (uint32_t)frames_in_flight);
                retire(k);                               // the slot's previous frames must be on disk before it is reused
                if(!started && f >= 0) { rr.finish_all(); t0 = std::chrono::high_resolution_clock::now(); started = true; }   // -t: the warm-up is over
                rr.render();
                in_slot[k] = f;
            }
            for(int n = 0; n < frames_in_flight; ++n) retire((int)((rr.frame_index / (uint32_t)B + n) % (uint32_t)frames_in_flight));
            if(timing)
            {
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
                const int counted = ((frames + B - 1) / B) * B;      // whole launches, like the loop above
                std::cout << "FRAMES " << counted << " (" << frames_in_flight << " in flight, " << B << " per launch): " << ms << " ms, " << ms / counted << " ms per frame\n";
            }
            return 0;
        }
        for(int f = -warmup; f < frames; ++f)
        {
            if(animated && f >= 0)
            {   // update(s, dt, true) before the frame, the first one by dt = 0; without --frames the run ends with the clip
                // (src/tauray.cc:1064-1092)
                if(!frames_given && !animator.is_playing()) break;
                animator.update(f == 0 ? 0 : update_dt);
                if(!frames_given && !animator.is_playing()) break;
                if(opt.taa) step_camera_jitter(scene);      // scene::update steps the jitter with the animation (src/scene.cc:228)
                rr.update_scene(scene, f % 3 == 2);      // an acceleration-structure update, every third frame a fast rebuild
            }
            else if(opt.taa) { step_camera_jitter(scene); rr.update_cameras(scene); }
            auto t0 = std::chrono::high_resolution_clock::now();
            rr.reset_accumulation();                   // offline frames: accumulation reset, sample counter kept (src/tauray.cc:1101)
            rr.render();
            rr.finish_frame();
            auto t1 = std::chrono::high_resolution_clock::now();
            if(f < 0) continue;
            if(timing)
            {   // print_simple_trace (src/tracing.cc:247-279)
                std::cout << "FRAME " << f << ":\n";
                std::vector<double> pt = rr.get_path_tracing_times();
                for(size_t i = 0; i < pt.size(); ++i)
                    std::cout << "\tDEVICE " << i << ":\n\t\t[path tracing (" << opt.active_viewport_count << " viewports)] " << pt[i] << " ms\n";
                std::cout << "\tHOST: " << std::chrono::duration<double, std::milli>(t1 - t0).count() << " ms\n";
            }
            out.save(*rr.per_device[0].dev, opt.looking_glass ? rr.composed : rr.display, (unsigned)f);
        }
        return 0;
        };
        if(renderer == "direct")
        {
            if(opt.bmfr) throw std::runtime_error("--denoiser=bmfr reads the path tracer's demodulated diffuse target: --renderer=path-tracer");
            if(opt.taa) throw std::runtime_error("--taa reads the path tracer's screen_motion target: --renderer=path-tracer");
            direct_renderer::options dopt;
            static_cast<path_tracer_stage::options&>(dopt) = opt;
            static_cast<post_processing_renderer::options&>(dopt) = opt;
            dopt.scene = opt.scene; dopt.accumulate = opt.accumulate; dopt.max_frames_in_flight = opt.max_frames_in_flight; dopt.frames_per_launch = opt.frames_per_launch;
            direct_renderer rr(devices, scene, size, dopt);
            return run(rr);
        }
        rt_renderer rr(devices, scene, size, opt);
        return run(rr);
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
