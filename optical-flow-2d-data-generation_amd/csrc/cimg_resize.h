// CImg<T>::get_resize(.., interpolation 3 = linear, boundary 0), enlarging branch, along one axis: destination pixel x of s
// reads source pixels at[x] and at[x] + 1 of len (len < s) with weight alpha[x] on the second.  CImg keeps running double
// sums; every rounding of them is restated here, once, for the host tables of the API layer.
#pragma once
#include <algorithm>

namespace ofdg {

template <typename Index>
inline void cimg_enlarge_table(int len, int s, Index* at, double* alpha) {
  const double f = s > 1 ? (len - 1.) / (s - 1) : 0;
  double curr = 0, old = 0;
  int pos = 0;
  for (int x = 0; x < s; ++x) {
    alpha[x] = curr - (unsigned int)curr;
    at[x] = (Index)pos;
    old = curr;
    curr = std::min(len - 1., curr + f);
    pos += (int)((unsigned int)curr - (unsigned int)old);
  }
}

}  // namespace ofdg
