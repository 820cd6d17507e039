// oracle/cvstub/opencv2/core/utility.hpp  --  TEST INFRASTRUCTURE ONLY (see ../core.hpp).  Included by the reference; nothing of it is used.
#ifndef CVSTUB_OPENCV2_CORE_UTILITY_HPP
#define CVSTUB_OPENCV2_CORE_UTILITY_HPP
#include "opencv2/core.hpp"
#endif
