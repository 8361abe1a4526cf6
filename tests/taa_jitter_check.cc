// The camera jitter of the C++ host (include/tauray_gltf.hh: get_camera_jitter_sequence, set_camera_jitter, step_camera_jitter).
// usage: taa_jitter_check <scene.glb> <width> <height> <sequence length> <steps>
// prints the sequence ("jitter x y" per entry, as float bit patterns), then per step the packed camera_data of every camera as hex,
// first as set_camera_jitter leaves them ("step 0"), then after each step_camera_jitter
#include "tauray_gltf.hh"
#include <cstdio>
#include <cstring>
int main(int argc, char** argv)
{
    if(argc < 6) return 2;
    try
    {
        const uint32_t w = (uint32_t)std::stoul(argv[2]), h = (uint32_t)std::stoul(argv[3]);
        const int n = std::stoi(argv[4]), steps = std::stoi(argv[5]);
        tr::scene_data scene = tr::load_glb(argv[1], w, h);
        const auto seq = tr::gltf_detail::get_camera_jitter_sequence(n, w, h);
        for(const auto& j: seq)
        {
            uint32_t bits[2];
            std::memcpy(bits, j.data(), 8);
            std::printf("jitter %08x %08x\n", bits[0], bits[1]);
        }
        tr::set_camera_jitter(scene, seq);
        for(int s = 0; s <= steps; ++s)
        {
            if(s) tr::step_camera_jitter(scene);
            std::printf("step %d ", s);
            for(uint8_t b: scene.cameras) std::printf("%02x", b);
            std::printf("\n");
        }
    }
    catch(const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}
