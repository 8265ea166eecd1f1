// Forwards to the stand-in (oracle/ref_shim/opencv2/opencv.hpp).
#include "../opencv.hpp"
