// Host-only check of the C++ host's deformation-motion plumbing (tr::scene_stage, include/tauray_hip.hh) for tests/test_deform_motion.py:
// needs no device.  The entry points of libtrhip that scene_stage::set_scene and scene_stage::apply call are defined here - the program's
// own definitions are the ones its calls bind to - and print their names, so the order of the calls can be read from the output.
//   deform_motion_check options        prints the defaults: scene_stage::options::deformation_motion rt_renderer::options::scene.deformation_motion
//   deform_motion_check order SWITCH   a scene stage made with the switch SWITCH (0 / 1) over a scene with one morphed and one skinned mesh:
//                                      set_scene, `--`, apply(s), `--`, apply(s, false, true), `--`, set_deformation_motion(true) and apply(s)
// Built by the test with the host sanitizers.
#include <cstdlib>
#include <iostream>
#include <string>

#include "tauray_hip.hh"

extern "C" {
struct trhip_device { int unused; };
static trhip_device the_device;
int trhip_device_create(int, trhip_device** out) { *out = &the_device; return 0; }
void trhip_device_destroy(trhip_device*) {}
const char* trhip_last_error(void) { return "stub"; }
int trhip_scene_upload(trhip_device*, const trhip_scene_desc*) { std::cout << "upload\n"; return 0; }
int trhip_scene_set_deformation_motion(trhip_device*, int on) { std::cout << "set_deformation_motion " << on << "\n"; return 0; }
int trhip_scene_latch_positions(trhip_device*) { std::cout << "latch\n"; return 0; }
int trhip_scene_set_skin(trhip_device*, uint32_t i, const void*, const trhip_skin*, uint32_t) { std::cout << "set_skin " << i << "\n"; return 0; }
int trhip_scene_skin(trhip_device*, uint32_t i, const float*, uint32_t) { std::cout << "skin " << i << "\n"; return 0; }
int trhip_scene_set_morph_targets(trhip_device*, uint32_t i, uint32_t, const float*, const float*, const float*, uint32_t) { std::cout << "set_morph_targets " << i << "\n"; return 0; }
int trhip_scene_morph(trhip_device*, uint32_t i, const float*, uint32_t) { std::cout << "morph " << i << "\n"; return 0; }
int trhip_scene_update_instances(trhip_device*, const void*, uint32_t) { std::cout << "update_instances\n"; return 0; }
int trhip_scene_update_cameras(trhip_device*, const void*, uint32_t) { std::cout << "update_cameras\n"; return 0; }
int trhip_scene_set_previous_cameras(trhip_device*, const void*, uint32_t) { std::cout << "set_previous_cameras\n"; return 0; }
int trhip_scene_update_lights(trhip_device*, const void*, uint32_t, const void*, uint32_t) { std::cout << "update_lights\n"; return 0; }
int trhip_scene_set_accel_strategy(trhip_device*, int) { return 0; }
int trhip_scene_set_dynamic_instances(trhip_device*, const uint8_t*, uint32_t) { return 0; }
int trhip_scene_set_build_mode(trhip_device*, int) { return 0; }
int trhip_scene_build_accel(trhip_device*, trhip_accel_info*) { std::cout << "build\n"; return 0; }
int trhip_scene_refit_accel(trhip_device*, trhip_accel_info*) { std::cout << "refit\n"; return 0; }
}

int main(int argc, char** argv)
{
    try
    {
        const std::string mode = argc > 1 ? argv[1] : "";
        if(mode == "options" && argc == 2)
        {
            std::cout << (tr::scene_stage::options().deformation_motion ? 1 : 0) << " " << (tr::rt_renderer::options().scene.deformation_motion ? 1 : 0) << "\n";
            return 0;
        }
        if(mode == "order" && argc == 3)
        {
            tr::scene_data s;
            s.instances.resize(2 * 288); s.spans.resize(2 * 16); s.vertices.resize(6 * 48); s.indices.resize(6 * 4); s.non_opaque.resize(2); s.cameras.resize(320);
            tr::scene_data::morphed_mesh mm;
            mm.instance = 0; mm.target_count = 1; mm.position_deltas.assign(9, 0.0f); mm.weights.assign(1, 0.5f);
            s.morphed.push_back(mm);
            tr::scene_data::skinned_mesh sk;
            sk.instance = 1; sk.skins.resize(3); sk.joint_transforms.assign(16, 0.0f);
            s.skinned.push_back(sk);
            tr::device dev(0);
            tr::scene_stage::options o;
            o.deformation_motion = std::atoi(argv[2]) != 0;
            tr::scene_stage ss(dev, o);
            ss.set_scene(s);
            std::cout << "--\n";
            ss.apply(s);
            std::cout << "--\n";
            ss.apply(s, false, true);
            std::cout << "--\n";
            ss.set_deformation_motion(true);
            ss.apply(s, true);
            return 0;
        }
        std::cerr << "usage: deform_motion_check options | order SWITCH\n";
        return 2;
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
