// Host-only check of ReSTIR DI's BSDF candidates for tests/test_restir_di_bsdf_candidates.py: the C++ host's option
// (tr::restir_di_stage::options::bsdf_candidates and parse_bsdf_candidates, include/tauray_hip.hh) and its check together with
// `candidates`.  Needs no device.
//   restir_bsdf_candidates_check parse TEXT [RESTIR]   parses --restir=RESTIR (when given) and --restir-bsdf-candidates=TEXT over the
//                                                      defaults, then the option check; prints "candidates bsdf_candidates"
//   restir_bsdf_candidates_check check L B             the stage's option check of candidates = L, bsdf_candidates = B; prints ok
//   restir_bsdf_candidates_check default               prints the default "candidates bsdf_candidates"
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
        if(mode == "parse" && (argc == 3 || argc == 4))
        {
            if(argc == 4) o.parse(argv[3]);
            o.parse_bsdf_candidates(argv[2]);
            o.check();
        }
        else if(mode == "check" && argc == 4)
        {
            o.candidates = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            o.bsdf_candidates = (uint32_t)std::strtoul(argv[3], nullptr, 10);
            o.check();
            std::cout << "ok\n";
            return 0;
        }
        else if(!(mode == "default" && argc == 2))
        {
            std::cerr << "usage: restir_bsdf_candidates_check parse TEXT [RESTIR] | check L B | default\n";
            return 2;
        }
        std::cout << o.candidates << " " << o.bsdf_candidates << "\n";
        return 0;
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
