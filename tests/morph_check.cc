// What tr::load_glb and tr::scene_animator make of a file's morph targets, printed for tests/test_morph_targets.py to hold against the
// Python loader and player.  No device: the loader and the player are host code.  Built with the host sanitizers by the test.
//   morph_check load FILE                   spans, then per morphed mesh: instance, node, targets, weights and the three planes (float bits)
//   morph_check play FILE FPS FRAMES        per frame the weights of every morphed mesh after scene_animator::update (float bits)
//   morph_check sample FILE NODE CLIP T...  the weights track of NODE's clip sampled at the given microsecond ticks (%.17g doubles)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "tauray_gltf.hh"

static void bits(const char* name, const std::vector<float>& v)
{
    std::printf("%s %zu", name, v.size());
    for(float f: v) { uint32_t u; std::memcpy(&u, &f, 4); std::printf(" %08x", u); }
    std::printf("\n");
}

int main(int argc, char** argv)
{
    try
    {
        if(argc < 3) throw std::runtime_error("usage: morph_check load|play|sample FILE ...");
        const std::string mode = argv[1];
        tr::scene_data s = tr::load_glb(argv[2], 48, 32);
        if(mode == "load")
        {
            const tr::gltf_detail::mesh_span* sp = reinterpret_cast<const tr::gltf_detail::mesh_span*>(s.spans.data());
            for(uint32_t i = 0; i < s.instance_count(); ++i) std::printf("span %u %u %u %u\n", sp[i].vertex_offset, sp[i].vertex_count, sp[i].index_offset, sp[i].triangle_count);
            std::printf("morphed %zu\n", s.morphed.size());
            for(const tr::scene_data::morphed_mesh& mm: s.morphed)
            {
                std::printf("mesh %u %d %u\n", mm.instance, mm.node, mm.target_count);
                bits("weights", mm.weights); bits("position", mm.position_deltas); bits("normal", mm.normal_deltas); bits("tangent", mm.tangent_deltas);
            }
        }
        else if(mode == "play" && argc >= 5)
        {
            tr::scene_animator an(s);
            an.play("");
            const double fps = std::atof(argv[3]);
            const int64_t dt = (int64_t)std::floor(1000000.0 / fps + 0.5);
            for(int f = 0; f < std::atoi(argv[4]); ++f)
            {
                an.update(f == 0 ? 0 : dt);
                for(const tr::scene_data::morphed_mesh& mm: s.morphed) bits("weights", mm.weights);
            }
        }
        else if(mode == "sample" && argc >= 5)
        {
            const tr::gltf_animation::track& t = s.animation->clips.at(std::atoi(argv[3])).at(argv[4]).weights;
            std::printf("loop_time %" PRId64 "\n", s.animation->clips.at(std::atoi(argv[3])).at(argv[4]).loop_time());
            for(int a = 5; a < argc; ++a)
            {
                const tr::gltf_animation::key v = t.sample(std::atoll(argv[a]), false);
                for(int k = 0; k < t.width; ++k) std::printf("%s%.17g", k ? " " : "", v[(size_t)k]);
                std::printf("\n");
            }
        }
        else throw std::runtime_error("unknown mode");
    }
    catch(const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}
