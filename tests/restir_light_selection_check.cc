// Host-only check of ReSTIR DI's power-proportional light selection for tests/test_restir_di_light_selection.py: the table builder the
// library uses (tr::build_light_alias_table, include/tauray_alias.hh) and the C++ host's option (tr::restir_di_stage::options::
// light_selection, uniform_fraction and parse_light_selection, include/tauray_hip.hh).  Needs no device.
//   restir_light_selection_check selftest                 the builder on tables derived by hand: n = 1, weights 1 : 3 at fraction 0.5, all zero; prints ok
//   restir_light_selection_check tables FILE FRACTION     FILE: records of { uint32 n; float weight[n]; }; per record one line, the table's
//                                                         entries as four 8-digit hex words each (alias_id, probability, pdf bits, alias_pdf bits)
//   restir_light_selection_check parse TEXT               parses --restir-light-selection=TEXT over the default, then the option check; prints "mode fraction"
//   restir_light_selection_check check MODE FRACTION      the stage's option check of light_selection = MODE, uniform_fraction = FRACTION; prints ok
//   restir_light_selection_check default                  prints the default "mode fraction"
// A refusal is printed to stderr and exits with 1.  Built by the test with the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "tauray_alias.hh"
#include "tauray_hip.hh"

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

static bool same(const tr::alias_entry& e, uint32_t alias_id, uint32_t probability, float pdf, float alias_pdf)
{
    return e.alias_id == alias_id && e.probability == probability && bits(e.pdf) == bits(pdf) && bits(e.alias_pdf) == bits(alias_pdf);
}

static int selftest()
{
    std::vector<tr::alias_entry> t(3);
    const float one[1] = {7.0f};
    tr::build_light_alias_table(one, 1, 0.1f, t.data());
    if(!same(t[0], 0, 0xFFFFFFFFu, 1.0f, 1.0f)) { std::cerr << "n = 1\n"; return 1; }
    // weights 1 : 3, fraction 0.5: p = 0.375, 0.625; n p = 0.75, 1.25: slot 0 keeps 0.75 = 0xC0000000 / 2^32 and spills into 1, which is left with exactly 1
    const float two[2] = {1.0f, 3.0f};
    tr::build_light_alias_table(two, 2, 0.5f, t.data());
    if(!same(t[0], 1, 0xC0000000u, 0.375f, 0.625f) || !same(t[1], 1, 0xFFFFFFFFu, 0.625f, 0.625f)) { std::cerr << "weights 1 : 3\n"; return 1; }
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    tr::build_light_alias_table(zero, 3, 0.25f, t.data());
    const float third = (float)(1.0 / 3.0);
    for(uint32_t k = 0; k < 3; ++k) if(!same(t[k], k, 0xFFFFFFFFu, third, third)) { std::cerr << "all zero\n"; return 1; }
    tr::build_light_alias_table(nullptr, 0, 0.1f, nullptr);      // an empty class touches nothing
    const std::vector<tr::alias_entry> both = tr::build_light_selection_table(two, 1, 1, 0.1f);      // two classes of one light each
    if(both.size() != 2 || !same(both[0], 0, 0xFFFFFFFFu, 1.0f, 1.0f) || !same(both[1], 0, 0xFFFFFFFFu, 1.0f, 1.0f)) { std::cerr << "two classes\n"; return 1; }
    std::cout << "ok\n";
    return 0;
}

int main(int argc, char** argv)
{
    try
    {
        const std::string mode = argc > 1 ? argv[1] : "";
        tr::restir_di_stage::options o;
        if(mode == "selftest" && argc == 2) return selftest();
        if(mode == "tables" && argc == 4)
        {
            std::ifstream f(argv[2], std::ios::binary);
            if(!f) throw std::runtime_error(std::string("Failed to open ") + argv[2]);
            const float fraction = std::strtof(argv[3], nullptr);
            uint32_t n = 0;
            while(f.read(reinterpret_cast<char*>(&n), 4))
            {
                std::vector<float> w(n);
                if(n && !f.read(reinterpret_cast<char*>(w.data()), std::streamsize(n) * 4)) throw std::runtime_error("truncated record");
                std::vector<tr::alias_entry> t(n);
                tr::build_light_alias_table(w.data(), n, fraction, t.data());
                std::string line;
                char word[40];
                for(const tr::alias_entry& e: t)
                {
                    std::snprintf(word, sizeof(word), "%08x%08x%08x%08x", e.alias_id, e.probability, bits(e.pdf), bits(e.alias_pdf));
                    line += word;
                }
                std::cout << line << "\n";
            }
            return 0;
        }
        if(mode == "parse" && argc == 3)
        {
            o.parse_light_selection(argv[2]);
            o.check();
            std::printf("%d %.9g\n", o.light_selection, o.uniform_fraction);
            return 0;
        }
        if(mode == "check" && argc == 4)
        {
            o.light_selection = (int)std::strtol(argv[2], nullptr, 10);
            o.uniform_fraction = std::strtof(argv[3], nullptr);
            o.check();
            std::cout << "ok\n";
            return 0;
        }
        if(mode == "default" && argc == 2)
        {
            std::printf("%d %.9g\n", o.light_selection, o.uniform_fraction);
            return 0;
        }
        std::cerr << "usage: restir_light_selection_check selftest | tables FILE FRACTION | parse TEXT | check MODE FRACTION | default\n";
        return 2;
    }
    catch(std::exception& e)
    {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
