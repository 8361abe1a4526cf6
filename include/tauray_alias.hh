// tauray_alias.hh - the 1-D alias table of ReSTIR DI's power-proportional light selection (csrc/restir_di.h `light selection`,
// DESIGN.md section 33): the one function libtrhip.so builds its table with, header-only and free of any other header of the project
// so that a stand-alone check (tests/restir_light_selection_check.cc) and both hosts can call the very same code.
// tests/restir_di_selection_model.py restates it in numpy, operation by operation.
//
// The work-list order and the threshold encoding are build_alias_table's (tauray_envmap.hh, after environment_map::generate_alias_table):
// i walks the slots at or below the average, j those above it, what is left of slot j spills into the next such slot.  One departure: the
// running weight and n * p_i are doubles here, not floats.  A float n * p_i alone is off by up to 2^-25 relative, 3e-8 of probability for
// a light that holds most of the power, and the table is asked to reproduce p_i to 2^-30; the environment table keeps its float steps and
// its bytes.
#ifndef TAURAY_ALIAS_HH
#define TAURAY_ALIAS_HH
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tr
{

struct alias_entry { uint32_t alias_id, probability; float pdf, alias_pdf; };      // 16 bytes: shader/alias_table.glsl:7-13, csrc/common.h AliasEntry
static_assert(sizeof(alias_entry) == 16, "alias entry layout");

// A weight that is negative, NaN or infinite counts as 0
inline float light_selection_clean_weight(float w) { return std::isfinite(w) && w > 0.0f ? w : 0.0f; }

// p_i = (1 - f) * w_i / sum(w) + f / n in double, sum(w) one running double sum in slot order; 1 / n when the sum is 0.
inline std::vector<double> light_selection_probabilities(const float* weights, size_t n, float uniform_fraction)
{
    std::vector<double> p(n);
    double total = 0;
    for(size_t i = 0; i < n; ++i) total += (double)light_selection_clean_weight(weights[i]);
    const double f = (double)uniform_fraction;
    for(size_t i = 0; i < n; ++i)
        p[i] = total > 0 ? (1.0 - f) * ((double)light_selection_clean_weight(weights[i]) / total) + f / (double)n : 1.0 / (double)n;
    return p;
}

// One class's table over its n slots: a draw takes slot = floor(u * n) with a uniform 32-bit word `low` beside it, and the slot's alias
// where low > probability.  pdf / alias_pdf are float(p) of the slot and of its alias.
inline void build_light_alias_table(const float* weights, size_t n, float uniform_fraction, alias_entry* table)
{
    const std::vector<double> p = light_selection_probabilities(weights, n, uniform_fraction);
    std::vector<double> importance(n);
    for(size_t i = 0; i < n; ++i) importance[i] = (double)n * p[i];
    for(size_t i = 0; i < n; ++i) table[i] = alias_entry{(uint32_t)i, 0xFFFFFFFFu, 0.0f, 0.0f};
    auto fixed32 = [](double v) {
        const double r = std::ldexp(v, 32);
        return (uint32_t)(r < 0.0 ? 0.0 : (r > 4294967295.0 ? 4294967295.0 : r));
    };
    size_t i = 0, j = 0;
    while(i < n && importance[i] > 1.0) ++i;
    while(j < n && importance[j] <= 1.0) ++j;
    double weight = j < n ? importance[j] : 0.0;
    while(j < n)
    {
        if(weight > 1.0)
        {
            if(i >= n) break;
            table[i].probability = fixed32(importance[i]);
            table[i].alias_id = (uint32_t)j;
            weight = (weight + importance[i]) - 1.0;
            ++i;
            while(i < n && importance[i] > 1.0) ++i;
        }
        else
        {
            table[j].probability = fixed32(weight);
            const size_t old_j = j;
            ++j;
            while(j < n && importance[j] <= 1.0) ++j;
            if(j < n)
            {
                table[old_j].alias_id = (uint32_t)j;
                weight = (weight + importance[j]) - 1.0;
            }
        }
    }
    for(size_t k = 0; k < n; ++k)
    {
        table[k].pdf = (float)p[k];
        table[k].alias_pdf = (float)p[table[k].alias_id];
    }
}

// The stage's table: the point lights' class, then the triangle lights', each over its own slots
inline std::vector<alias_entry> build_light_selection_table(const float* weights, size_t n_point, size_t n_tri, float uniform_fraction)
{
    std::vector<alias_entry> table(n_point + n_tri);
    build_light_alias_table(weights, n_point, uniform_fraction, table.data());
    build_light_alias_table(weights + n_point, n_tri, uniform_fraction, table.data() + n_point);
    return table;
}

}
#endif
