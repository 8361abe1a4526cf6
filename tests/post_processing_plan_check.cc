// The plan of the C++ host's post-processing chain (include/tauray_hip.hh: post_processing_renderer::make_plan) for every on/off combination
// of denoiser, spatial reprojection, temporal reprojection, taa and a Looking Glass output on one device with 8 viewports, 3 of them sources.
// No device is touched.  Prints one line per combination:
//   <d> <s> <t> <a> <l> plan <stages,comma separated> <targets,comma separated or -> <frame_order> <fused_tonemap> <output_layers>
//   <d> <s> <t> <a> <l> refused <what()>
#include "tauray_hip.hh"
#include <cstdio>
static std::string join(const std::vector<std::string>& v)
{
    std::string out;
    for(const std::string& s: v) out += (out.empty() ? "" : ",") + s;
    return out.empty() ? "-" : out;
}
int main()
{
    using ppr = tr::post_processing_renderer;
    for(int row = 0; row < 32; ++row)
    {
        const bool d = row & 16, s = row & 8, t = row & 4, a = row & 2, l = row & 1;
        ppr::options opt;
        if(d) opt.bmfr = tr::bmfr_stage::options{};
        if(s) opt.spatial_reprojection = {0, 3, 6};
        if(t) opt.temporal_reprojection = 0.5f;
        if(a) opt.taa = ppr::options::taa_options{};
        if(l) { ppr::options::looking_glass_options lo; lo.stage.viewport_count = 8; lo.output_size = {96, 128}; opt.looking_glass = lo; }
        ppr::facts facts;
        facts.viewports = 8;
        std::printf("%d %d %d %d %d ", d, s, t, a, l);
        try
        {
            const ppr::plan p = ppr::make_plan(opt, facts);
            std::printf("plan %s %s %d %d %zu\n", join(p.stages).c_str(), join(p.targets).c_str(), p.frame_order, p.fused_tonemap, p.output_layers);
        }
        catch(const std::exception& e) { std::printf("refused %s\n", e.what()); }
    }
    return 0;
}
