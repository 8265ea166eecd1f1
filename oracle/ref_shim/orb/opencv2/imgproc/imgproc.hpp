// part of the stand-in OpenCV of ref_orb: everything is in core/core.hpp
#include "../core/core.hpp"
