// cascade_model.h -- a cascade as the loader (cascade_xml.cpp) leaves it: plain C++, no HIP.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include "../../include/nubovca.h"

namespace nvca {

// --------------------------------------------------------------------------
// Cascade as loaded from old-format XML (OpenCV CvHaarClassifierCascade).
// --------------------------------------------------------------------------
struct HaarNode {
    int   rect[3][4];   // x,y,w,h ; zero when absent
    float weight[3];
    int   nrect;        // 2 or 3 (icvCreateHidHaarClassifierCascade's rect[2] test)
    float threshold;
    int   left, right;  // >0 child node index, <=0 -> alpha[-idx]
    int   tilted;
};
struct HaarClassifier { int first_node, nnodes, first_alpha; };
struct HaarStage { int first_cls, ncls; float threshold; /* as in the XML */ };

struct Cascade {
    int ow = 0, oh = 0;
    std::vector<HaarStage> stages;
    std::vector<HaarClassifier> cls;
    std::vector<HaarNode> nodes;
    std::vector<float> alpha;
    bool stump_based = true;
    bool has_tilted = false; // some feature reads the tilted integral
    bool generic() const { return !stump_based || has_tilted; }   // evaluated by the general kernels (kernels_cascade_gather.hip)
    uint64_t uid = 0;       // identity for plan caching
    mutable std::vector<unsigned char> stage_rec_cache;   // StageRec[] (plan.cpp, built on first use: the summation-order proof is per cascade)
};

// --------------------------------------------------------------------------
// Cascade as loaded from new-format XML (type_id="opencv-cascade-classifier"), featureType LBP, stump weak classifiers:
// what OpenCV 2.4 cascadedetect.cpp (CascadeClassifier::Data::read, LBPEvaluator::read) keeps.  SURVEY.md A.15.
// --------------------------------------------------------------------------
struct LbpFeature { int x, y, w, h; };          // top-left cell of the 3 x 3 grid of w x h cells, window-relative
struct LbpWeak { int feature; int32_t subset[8]; float leaf[2]; };      // vote = subset[code >> 5] & (1 << (code & 31)) ? leaf[0] : leaf[1]
struct LbpStage { int first, count; float threshold; /* as evaluated: (float)value - 1e-5f */ };
struct LbpCascade {
    int ow = 0, oh = 0;
    std::vector<LbpFeature> features;
    std::vector<LbpWeak> weak;
    std::vector<LbpStage> stages;
};

// --------------------------------------------------------------------------
// The same envelope with featureType HAAR: what Data::read and HaarEvaluator::read keep of a cascade of stumps on upright features.
// SURVEY.md A.16.  A feature has one to three rects; a missing one is all zero with weight 0 (its sum is 0, the third is not added).
// --------------------------------------------------------------------------
struct HnewFeature { int rect[3][4]; float weight[3]; int nrect; };      // x, y, w, h, window-relative
struct HnewWeak { int feature; float threshold; float leaf[2]; };        // vote = value < threshold ? leaf[0] : leaf[1]
// A general cascade (loaded with NVCA_LOAD_HAAR_GENERAL from a file that holds a tree or a tilted feature): a weak
// classifier is a tree of 1 .. kHgenMaxNodes nodes, in file order with every child node behind its parent; a child > 0 is a node of the
// same tree, a child <= 0 its leaf -child.  `weak` is empty then; a stage's first / count index `trees`.
static constexpr int kHgenMaxNodes = 15;      // nodes of one weak classifier (a depth-4 tree is full at 15)
struct HgenNode { int left, right, feature; float threshold; };
struct HgenTree { int first_node, nnodes, first_leaf; };          // nnodes + 1 leaves from first_leaf
struct HnewCascade {
    int ow = 0, oh = 0;
    std::vector<HnewFeature> features;
    std::vector<HnewWeak> weak;
    std::vector<LbpStage> stages;          // (threshold as evaluated: (float)value - 1e-5f, as an LBP cascade's)
    bool general = false;                  // trees / nodes / leaves / tilted hold the weak classifiers (kernels_cascade_hgen.hip evaluates them)
    std::vector<HgenTree> trees;
    std::vector<HgenNode> nodes;
    std::vector<float> leaves;
    std::vector<unsigned char> tilted;     // per feature: all of its rects read the tilted integral
    bool has_tilted = false;
    size_t nweak() const { return general ? trees.size() : weak.size(); }
};

// a cascade file of either format: `format` says which model the loader filled (haar.ow / haar.oh hold the window either way)
struct CascadeFile { int format = NVCA_CASCADE_HAAR; Cascade haar; LbpCascade lbp; HnewCascade hnew; };

// returns NVCA_OK or NVCA_ERR_PARSE / NVCA_ERR_UNSUPPORTED; err gets a message
int parse_cascade_xml(const char *text, size_t len, Cascade &out, std::string &err);      // old-format files only
int parse_cascade_file(const char *text, size_t len, CascadeFile &out, std::string &err); // both formats, by the type_id of the first child of <opencv_storage>
// the same with load flags (NVCA_LOAD_*; 0: the call above): NVCA_LOAD_HAAR_GENERAL admits trees and tilted features in a new-format HAAR file
int parse_cascade_file(const char *text, size_t len, unsigned flags, CascadeFile &out, std::string &err);

} // namespace nvca
