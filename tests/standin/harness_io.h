// What the script-driven harnesses (tests/*_dropin/harness.cpp) share: the readers of their script tokens and the out-of-class definitions the stand-in
// classes of this directory leave open.  Those definitions are not inline (the drop-in objects call them), so a harness includes this header in its
// one translation unit.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"

namespace ORB_SLAM {

float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
int Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
int MapPoint::nReplaced = 0;

// src/MapPoint.cc:141-176 without the descriptor update and the map's bookkeeping
void MapPoint::Replace(MapPoint* pMP) {
    if (pMP->mnId == mnId) return;
    nReplaced++;
    const std::map<KeyFrame*, std::size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    for (std::map<KeyFrame*, std::size_t>::const_iterator mit = obs.begin(); mit != obs.end(); ++mit) {
        KeyFrame* pKF = mit->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF, mit->second);
        } else {
            pKF->EraseMapPointMatch(mit->second);
        }
    }
}

void MapPoint::EraseObservation(KeyFrame* pKF) {
    if (mObservations.erase(pKF) == 0) return;
    if (mObservations.size() <= 2) SetBadFlag();
}

void MapPoint::SetBadFlag() {
    mbBad = true;
    std::map<KeyFrame*, std::size_t> obs;
    obs.swap(mObservations);
    for (std::map<KeyFrame*, std::size_t>::iterator it = obs.begin(); it != obs.end(); ++it) it->first->EraseMapPointMatch(it->second);
}

}  // namespace ORB_SLAM

// a float travels as the hex of its bit pattern
inline float rdf(std::istringstream& in) {
    std::string h;
    in >> h;
    const uint32_t u = (uint32_t)strtoul(h.c_str(), nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// a descriptor travels as 64 hex digits
inline void rddesc(std::istringstream& in, unsigned char* d) {
    std::string h;
    in >> h;
    for (int i = 0; i < 32; i++) d[i] = (unsigned char)strtoul(h.substr(i * 2, 2).c_str(), nullptr, 16);
}
