// A DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned int> >) as the CSR the device reads (include/orbs.h, the layout
// orbv_transform_batch_device writes): node ids ascending, which is the map's order, one offset per node, the features in their vector's order.
#pragma once
#include <cstdint>

namespace ORB_SLAM {

// node[cap], off[cap + 1], feat[cap] -> the number of nodes; -1 when the vector does not fit `cap` nodes or features, or names a feature
// outside [0, nfeatures)
template <class FeatureVector>
int PackFeatureVector(const FeatureVector& fv, int nfeatures, int cap, uint32_t* node, int32_t* off, uint32_t* feat) {
    int nn = 0, nf = 0;
    off[0] = 0;
    for (typename FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        if (nn >= cap) return -1;
        for (std::size_t j = 0; j < it->second.size(); j++) {
            const unsigned f = it->second[j];
            if (f >= (unsigned)nfeatures || nf >= cap) return -1;
            feat[nf++] = f;
        }
        node[nn++] = (uint32_t)it->first;
        off[nn] = nf;
    }
    return nn;
}

}  // namespace ORB_SLAM
