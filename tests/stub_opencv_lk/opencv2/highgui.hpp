// NOT OpenCV: see opencv2/core.hpp of this directory (a stand-in for the names the reference's lkpyramid files use)
#pragma once
#include <opencv2/core.hpp>
