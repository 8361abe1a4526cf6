// Host-only check of the C++ host's ReSTIR GI options (tr::restir_gi_stage::options, include/tauray_hip.hh) for tests/test_restir_gi.py:
// needs no device.
//   restir_gi_check parse TEXT                     parses --restir-gi=TEXT over the defaults and prints
//                                                  spatial_samples search_radius max_confidence temporal_reuse
//   restir_gi_check check S RADIUS CONFIDENCE MIN  the renderer's option check of these values; prints ok
// A refusal is printed to stderr and exits with 1.  Built by the test with the host sanitizers.
#include <cstdlib>
#include <iostream>
#include <string>

#include "tauray_hip.hh"

int main(int argc, char** argv)
{
    try
    {
        const std::string mode = argc > 1 ? argv[1] : "";
        tr::restir_gi_stage::options o;
        if(mode == "parse" && argc == 3)
        {
            o.parse(argv[2]);
            std::cout << o.spatial_samples << " " << o.search_radius << " " << o.max_confidence << " " << (o.temporal_reuse ? 1 : 0) << "\n";
            return 0;
        }
        if(mode == "check" && argc == 6)
        {
            o.spatial_samples = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            o.search_radius = std::strtof(argv[3], nullptr); o.max_confidence = std::strtof(argv[4], nullptr); o.min_ray_dist = std::strtof(argv[5], nullptr);
            o.check();
            std::cout << "ok\n";
            return 0;
        }
        std::cerr << "usage: restir_gi_check parse TEXT | check S RADIUS CONFIDENCE MIN\n";
        return 2;
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
