// Stand-in ORB_SLAM::Map for the BundleAdjuster drop-in harness: the two lists GlobalBundleAdjustemnt asks for (include/Map.h).
#pragma once
#include <vector>

namespace ORB_SLAM {

class KeyFrame;
class MapPoint;

class Map {
public:
    std::vector<KeyFrame*> mvpKeyFrames;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> GetAllKeyFrames() { return mvpKeyFrames; }
    std::vector<MapPoint*> GetAllMapPoints() { return mvpMapPoints; }
};

}  // namespace ORB_SLAM
