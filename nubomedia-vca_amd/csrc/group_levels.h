// group_levels.h -- cv::groupRectangles(rectList, rejectLevels, levelWeights, groupThreshold, eps): the grouping of
// detectMultiScale with outputRejectLevels.  Pure host code: no HIP, no context (group_levels.cpp).
#pragma once
#include <vector>
#include "../../include/nubovca.h"

namespace nvca {

// In place on three parallel lists.  The classes and their averaged rectangles are group_rectangles' (host_logic.cpp: group_classes).
// Per class: maxLevel, the largest level of a member (from 0), and maxWeight (from DBL_MIN) -- a member with a greater level replaces
// both, one with an equal level replaces the weight when its own is greater.  A class is kept by its maxLevel, NOT by its member count
// (dropped when maxLevel <= groupThreshold); the contained-box filter still reads the OTHER class's member count.  A kept class answers
// with its averaged rectangle, maxLevel and maxWeight, in class order.
// groupThreshold <= 0 leaves the three lists untouched: the library's choice (OpenCV 2.4's early return there is not remembered with
// certainty).  The lists must have one length; otherwise nothing is done and false is returned.
bool group_rectangles_levels(std::vector<nvca_rect> &rects, std::vector<int> &levels, std::vector<double> &weights, int groupThreshold, double eps);

} // namespace nvca
