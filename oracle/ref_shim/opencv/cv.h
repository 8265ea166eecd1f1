// Forwards to the stand-in (oracle/ref_shim/opencv2/opencv.hpp): the reference's include/ORBextractor.h asks for the old name.
#include "../opencv2/opencv.hpp"
