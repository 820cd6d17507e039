// oracle/cvstub/opencv2/opencv.hpp  --  TEST INFRASTRUCTURE ONLY (see core.hpp).  The umbrella header StitchTool.hpp includes.
#ifndef CVSTUB_OPENCV2_OPENCV_HPP
#define CVSTUB_OPENCV2_OPENCV_HPP
#include "opencv2/core.hpp"
#include "opencv2/imgproc.hpp"
#endif
