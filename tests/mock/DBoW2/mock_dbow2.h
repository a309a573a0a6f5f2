// Stand-ins for the two DBoW2 container types ORBVocabulary::transform fills (the image has no DBoW2 headers): what matters to include/plf.hpp is
// that a BowVector is an ordered map word id -> value and a FeatureVector an ordered map node id -> feature indices.  Test scaffolding only.
#pragma once
#include <map>
#include <vector>

namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;

class BowVector : public std::map<WordId, WordValue> {};
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {};
}  // namespace DBoW2
