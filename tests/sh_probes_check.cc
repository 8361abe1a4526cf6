// The light-probe grids of the C++ host (include/tauray_gltf.hh: TR_data.light_probe; include/tauray_hip.hh: sh_grid, sh_grid_parameters).
// usage: sh_probes_check gltf <scene.gltf>
//   prints per grid: the resolution, the radius, the transform (column-major) and the scaling, as decimal numbers
// usage: sh_probes_check params <rx> <ry> <rz> <samples per probe> <first frame counter> <temporal ratio> <16 transform, column-major> <3 scaling>
//   prints, for three consecutive renders of a new stage, what the host packs for the grid: transform (16), normal transform (9, column-major
//   3 x 3), cell_scale (3), rotation_x, rotation_y, mix_ratio - one line per render, every number as a hexadecimal float
#include "tauray_gltf.hh"
#include <cstdio>
#include <cstring>
int main(int argc, char** argv)
{
    if(argc < 3) return 2;
    try
    {
        if(!std::strcmp(argv[1], "gltf"))
        {
            const tr::scene_data scene = tr::load_glb(argv[2], 64, 64);
            for(const tr::sh_grid& g: scene.sh_grids)
            {
                std::printf("%u %u %u %.9g", g.resolution[0], g.resolution[1], g.resolution[2], g.radius);
                for(float v: g.transform) std::printf(" %.9g", v);
                for(float v: g.scaling) std::printf(" %.9g", v);
                std::printf("\n");
            }
            return 0;
        }
        if(std::strcmp(argv[1], "params") || argc < 8 + 19) return 2;
        tr::sh_grid g;
        for(int i = 0; i < 3; ++i) g.resolution[i] = (uint32_t)std::stoul(argv[2 + i]);
        const uint32_t samples = (uint32_t)std::stoul(argv[5]), frame = (uint32_t)std::stoul(argv[6]);
        const float ratio = std::stof(argv[7]);
        for(int i = 0; i < 16; ++i) g.transform[i] = std::stof(argv[8 + i]);
        for(int i = 0; i < 3; ++i) g.scaling[i] = std::stof(argv[24 + i]);
        for(uint32_t k = 0; k < 3; ++k)
        {
            const trhip_sh_grid_data d = tr::sh_grid_parameters(g, samples, frame + k, k + 1, ratio);
            for(float v: d.transform) std::printf("%a ", v);
            for(int c = 0; c < 3; ++c) for(int r = 0; r < 3; ++r) std::printf("%a ", d.normal_transform[4 * c + r]);
            for(float v: d.cell_scale) std::printf("%a ", v);
            std::printf("%a %a %a\n", d.rotation_x, d.rotation_y, d.mix_ratio);
        }
    }
    catch(const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}
