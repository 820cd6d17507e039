// oracle/cvstub/opencv2/highgui.hpp  --  TEST INFRASTRUCTURE ONLY (see core.hpp).  The reference includes this header; the files compiled
// against the stand-in (everything but main.cpp and util.cpp) use nothing from it.
#ifndef CVSTUB_OPENCV2_HIGHGUI_HPP
#define CVSTUB_OPENCV2_HIGHGUI_HPP
#include "opencv2/core.hpp"
#endif
