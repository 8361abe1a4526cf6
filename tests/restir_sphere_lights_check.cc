// Host-only check of ReSTIR DI's sphere lights mode for tests/test_restir_di_sphere_lights.py: the C++ host's option
// (tr::restir_di_stage::options::sphere_lights and parse_sphere_lights, include/tauray_hip.hh) and its check.  Needs no device.
//   restir_sphere_lights_check parse TEXT   parses --restir-sphere-lights=TEXT over the defaults, then the option check; prints the mode
//   restir_sphere_lights_check check MODE   the stage's option check of sphere_lights = MODE (a number); prints ok
//   restir_sphere_lights_check default      prints the default mode
// A refusal is printed to stderr and exits with 1.  Built by the test with the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "tauray_hip.hh"

int main(int argc, char** argv)
{
    try
    {
        const std::string mode = argc > 1 ? argv[1] : "";
        tr::restir_di_stage::options o;
        if(mode == "parse" && argc == 3)
        {
            o.parse_sphere_lights(argv[2]);
            o.check();
        }
        else if(mode == "check" && argc == 3)
        {
            o.sphere_lights = (int)std::strtol(argv[2], nullptr, 10);
            o.check();
            std::cout << "ok\n";
            return 0;
        }
        else if(!(mode == "default" && argc == 2))
        {
            std::cerr << "usage: restir_sphere_lights_check parse TEXT | check MODE | default\n";
            return 2;
        }
        std::cout << o.sphere_lights << "\n";
        return 0;
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
