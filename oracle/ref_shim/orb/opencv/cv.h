// part of the stand-in OpenCV of ref_orb: everything is in opencv2/core/core.hpp
#include "../opencv2/core/core.hpp"
