// The names and ranges of Blender 3.6's view settings, as host data: the looks
// of the Filmic view, the view transforms' names, the ranges of the display
// gamma and the dither. No HIP header: the scene loader (scene.cpp) and the
// output settings (settings.cpp) need nothing else of view.hpp, which has the
// chain these belong to and where it comes from.
#pragma once

#include <string>

#include "rr.h"

namespace rr {

// Blender 3.6's looks of the Filmic view and the 1D curve each puts in the
// base curve's place. file nullptr: the base curve itself (no extra file).
// A look's id is its index here; 0 is "None".
struct LookDef {
    const char* name;
    const char* file;
};
constexpr int kNumLooks = 8;
constexpr LookDef kLooks[kNumLooks] = {
    {"None", nullptr},
    {"Very High Contrast", "filmic_to_1.20_1-00.spi1d"},
    {"High Contrast", "filmic_to_0.99_1-0075.spi1d"},
    {"Medium High Contrast", "filmic_to_0-85_1-011.spi1d"},
    {"Medium Contrast", nullptr},  // filmic_to_0-70_1-03.spi1d, the base curve
    {"Medium Low Contrast", "filmic_to_0-60_1-04.spi1d"},
    {"Low Contrast", "filmic_to_0-48_1-09.spi1d"},
    {"Very Low Contrast", "filmic_to_0-35_1-30.spi1d"},
};
constexpr const char* kFalseColorFile = "filmic_false_color.spi3d";
// Blender's range of view_settings.gamma
constexpr float kGammaMax = 5.0f;
// Blender's range of image_settings.dither_intensity: [0, kDitherMax]
constexpr float kDitherMax = 2.0f;

// The id of a look by its name, with or without Blender's "Filmic - " prefix;
// -1 for a name that is not in kLooks.
inline int look_id(const std::string& name) {
    const std::string prefix = "Filmic - ";
    const std::string n = name.rfind(prefix, 0) == 0 ? name.substr(prefix.size()) : name;
    for (int id = 0; id < kNumLooks; ++id)
        if (n == kLooks[id].name) return id;
    return -1;
}

// Blender's name of a view transform this renderer knows ("Standard", ...,
// "False Color").
inline const char* view_name(int view_transform) {
    switch (view_transform) {
    case RR_VIEW_STANDARD: return "Standard";
    case RR_VIEW_RAW: return "Raw";
    case RR_VIEW_FILMIC: return "Filmic";
    case RR_VIEW_FILMIC_LOG: return "Filmic Log";
    case RR_VIEW_FALSE_COLOR: return "False Color";
    default: return "?";
    }
}

}  // namespace rr
