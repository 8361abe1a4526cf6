// The Looking Glass rig of the C++ host (include/tauray_gltf.hh: looking_glass_calibration, looking_glass_cameras, the rig under scene_animator).
// usage: looking_glass_cameras_check <scene.glb> <view width> <view height> <viewports> <midplane> <depth> <relative_dist>
//                                    <pitch> <slope> <center> <viewCone> <invView> <DPI> <screenW> <screenH> <animation updates>
// prints "calibration <corrected_pitch> <tilt>" as float bit patterns, then "step 0 <hex>": the packed camera_data of every view as
// looking_glass_cameras leaves them, then the same after each update of the scene's animation at 60 frames per second (the first by dt = 0)
#include "tauray_gltf.hh"
#include <cstdio>
#include <cstring>
int main(int argc, char** argv)
{
    if(argc < 17) return 2;
    try
    {
        const uint32_t w = (uint32_t)std::stoul(argv[2]), h = (uint32_t)std::stoul(argv[3]);
        const uint32_t viewports = (uint32_t)std::stoul(argv[4]);
        const double midplane = std::stod(argv[5]), depth = std::stod(argv[6]), relative_dist = std::stod(argv[7]);
        tr::looking_glass_calibration cal;
        cal.pitch = (float)std::stod(argv[8]); cal.slope = (float)std::stod(argv[9]); cal.center = (float)std::stod(argv[10]);
        cal.view_cone = (float)std::stod(argv[11]); cal.invert = std::stoi(argv[12]) != 0; cal.dpi = (float)std::stod(argv[13]);
        cal.screen_w = (uint32_t)std::stoul(argv[14]); cal.screen_h = (uint32_t)std::stoul(argv[15]);
        const int updates = std::stoi(argv[16]);
        tr::scene_data scene = tr::load_glb(argv[1], w, h);
        const float derived[2] = {cal.corrected_pitch(), cal.tilt()};
        uint32_t bits[2];
        std::memcpy(bits, derived, 8);
        std::printf("calibration %08x %08x\n", bits[0], bits[1]);
        if(tr::looking_glass_cameras(scene, viewports, midplane, depth, relative_dist, cal) != viewports) return 3;
        tr::scene_animator animator(scene);
        animator.play("", false);
        for(int s = 0; s <= updates; ++s)
        {
            if(s) animator.update(s == 1 ? 0 : 16667);
            std::printf("step %d ", s);
            for(uint8_t b: scene.cameras) std::printf("%02x", b);
            std::printf("\n");
        }
    }
    catch(const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}
