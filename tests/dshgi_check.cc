// Host-only check of the C++ host's grid pick (tr::dshgi_pick_grid, include/tauray_hip.hh) for tests/test_dshgi.py: needs no device.
//   dshgi_check pick scene.gltf x y z [x y z ...]   prints the index of the grid each position shades from, in the loader's grid order
// Built by the test with the host sanitizers.
#include <cstdlib>
#include <iostream>
#include <string>

#include "tauray_hip.hh"
#include "tauray_gltf.hh"

int main(int argc, char** argv)
{
    try
    {
        if(argc < 3 || std::string(argv[1]) != "pick" || (argc - 3) % 3 != 0) { std::cerr << "usage: dshgi_check pick scene.gltf x y z ...\n"; return 2; }
        const tr::scene_data scene = tr::load_glb(argv[2], 64, 64);
        for(int i = 3; i + 2 < argc; i += 3)
        {
            const float p[3] = {std::strtof(argv[i], nullptr), std::strtof(argv[i + 1], nullptr), std::strtof(argv[i + 2], nullptr)};
            std::cout << tr::dshgi_pick_grid(scene.sh_grids, p) << "\n";
        }
        return 0;
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
