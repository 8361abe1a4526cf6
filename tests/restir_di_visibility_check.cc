// Host-only check of the C++ host's ReSTIR DI visibility option (tr::restir_di_stage::options::visibility and parse_visibility,
// include/tauray_hip.hh) for tests/test_restir_di_visibility.py: needs no device.
//   restir_di_visibility_check parse TEXT   parses --restir-visibility=TEXT over the default and prints the mode, then the option check's verdict
//   restir_di_visibility_check check MODE   the stage's option check of visibility = MODE (an integer); prints ok
//   restir_di_visibility_check default      prints the default mode
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
        tr::restir_di_stage::options o;
        if(mode == "parse" && argc == 3)
        {
            o.parse_visibility(argv[2]);
            o.check();
            std::cout << o.visibility << "\n";
            return 0;
        }
        if(mode == "check" && argc == 3)
        {
            o.visibility = (int)std::strtol(argv[2], nullptr, 10);
            o.check();
            std::cout << "ok\n";
            return 0;
        }
        if(mode == "default" && argc == 2)
        {
            std::cout << o.visibility << "\n";
            return 0;
        }
        std::cerr << "usage: restir_di_visibility_check parse TEXT | check MODE | default\n";
        return 2;
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
