// Ring bookkeeping of the scan log (vba_scanlog_*): where a scan goes in an arena of `cap` points that is used as a
// ring of WHOLE scans, when the arena's tail is skipped, when the arena is full, what a release frees and how a growth re-bases
// the live scans.  Host code only, the standard library only: no runtime call, no pointer into the arena.  Tested stand-alone
// (tests/host/scanlog_host.cpp).
//
// Live scans are numbered first() .. end() - 1 and lie in push order.  head = one past the newest scan's last point, tail = the
// oldest scan's first point (both 0 while nothing is live).  A scan never straddles the arena's end, so consecutive scans need not
// be contiguous: a reader takes every scan's own start().
//   not wrapped (starts ascend):       free = [head, cap) and [0, tail)
//   wrapped (a push skipped the tail and the oldest scan still lies above the newest): free = [head, tail); the points
//                                      [top, cap) that the push skipped stay unusable until a release takes the oldest scan past them
// place(n): an empty scan goes to head and takes no room.  Otherwise, not wrapped: head when head + n <= cap, else 0 when n <= tail
// (the tail is skipped), else full; wrapped: head when head + n <= tail, else full.  With nothing live the ring is rewound, so a scan
// of n <= cap points always fits.  In words: a push fits when
//     live points + the gap at the arena's end (of the wrap in force, or the one this push would leave) + n  <=  cap
// and the live scans, this one included, stay within scan_cap().  That is the condition of vba_scanlog_reserve (include/voxelba.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vba {

struct ScanRing {
  struct Scan { int64_t start, n; };
  struct Move { int64_t from, to, n; };      // a live scan's points on their way into a grown arena

  int64_t cap() const { return cap_; }
  int64_t first() const { return first_; }
  int64_t end() const { return first_ + (int64_t)count_; }
  size_t scans() const { return count_; }
  size_t scan_cap() const { return q_.size(); }
  bool live(int64_t seq) const { return seq >= first_ && seq < end(); }
  // [first, first + k) lies wholly inside the live range (k >= 0)
  bool live_range(int64_t first, int64_t k) const { return k >= 0 && first >= first_ && first <= end() && k <= end() - first; }
  const Scan &at(int64_t seq) const { return q_[(qhead_ + (size_t)(seq - first_)) % q_.size()]; }
  int64_t start(int64_t seq) const { return at(seq).start; }
  int64_t size(int64_t seq) const { return at(seq).n; }
  int64_t live_points() const { return live_; }
  int64_t head() const { return count_ ? at(end() - 1).start + at(end() - 1).n : 0; }
  int64_t tail() const { return count_ ? at(first_).start : 0; }
  bool wrapped() const { return wrap_; }

  // room for `scans` live scans; the records move, the numbers and starts stay
  void reserve_scans(size_t scans) {
    if (scans <= q_.size()) return;
    std::vector<Scan> nq(scans);
    for (size_t i = 0; i < count_; i++) nq[i] = q_[(qhead_ + i) % q_.size()];
    q_.swap(nq);
    qhead_ = 0;
  }
  // the arena's size as the caller allocated it; with live scans only through rebase()
  void set_cap(int64_t cap) { cap_ = cap; }

  // where a scan of n points would start, or -1 when the arena is full (the scan table is not looked at)
  int64_t place(int64_t n) const {
    if (n < 0) return -1;
    if (live_ == 0 && n > 0) return n <= cap_ ? 0 : -1;            // rewound: only empty scans are live, they hold no room
    const int64_t h = head(), t = tail();
    if (n == 0) return h;
    if (wrapped()) return h + n <= t ? h : -1;
    if (h + n <= cap_) return h;
    return n <= t ? 0 : -1;                                         // the tail [h, cap) is skipped
  }
  bool table_full() const { return count_ == q_.size(); }
  bool fits(int64_t n) const { return !table_full() && place(n) >= 0; }

  // appends the scan at place(n) (the caller has made sure that fits(n)); returns its number
  int64_t push(int64_t n) {
    const int64_t s = place(n);
    if (live_ == 0 && n > 0) {                                      // the rewind moves the live empty scans to 0 with it
      for (size_t i = 0; i < count_; i++) q_[(qhead_ + i) % q_.size()].start = 0;
      wrap_ = false;
    } else if (n > 0 && s < head()) {
      wrap_ = true;                                                 // the tail is skipped
    }
    q_[(qhead_ + count_) % q_.size()] = Scan{s, n};
    count_++;
    live_ += n;
    return end() - 1;
  }

  // drops every scan with seq < upto; returns how many went
  int64_t release(int64_t upto) {
    int64_t gone = 0;
    while (count_ && first_ < upto) {
      const int64_t was = q_[qhead_].start;
      live_ -= q_[qhead_].n;
      qhead_ = (qhead_ + 1) % q_.size();
      count_--; first_++; gone++;
      // the scan the wrapping push wrote starts at 0, below every scan of the arena's upper part: the oldest scan is past the wrap
      if (!count_ || q_[qhead_].start < was) wrap_ = false;
    }
    return gone;
  }

  // the arena after a push of n points that does not fit: cap doubled (an empty arena: `floor`) until it holds the live points
  // and n more, packed
  int64_t grown_cap(int64_t n, int64_t floor) const {
    int64_t m = cap_ > 0 ? 2 * cap_ : (floor > 0 ? floor : 1);
    while (m < live_ + n) m *= 2;
    return m;
  }
  // the arena becomes newcap points (>= live points): the live scans are packed from 0 in order, numbers kept; moves = what to copy
  void rebase(int64_t newcap, std::vector<Move> *moves) {
    int64_t at0 = 0;
    for (size_t i = 0; i < count_; i++) {
      Scan &s = q_[(qhead_ + i) % q_.size()];
      if (moves && s.n > 0) moves->push_back(Move{s.start, at0, s.n});
      s.start = at0;
      at0 += s.n;
    }
    wrap_ = false;
    cap_ = newcap;
  }

 private:
  int64_t cap_ = 0, first_ = 0, live_ = 0;
  std::vector<Scan> q_;          // circular: qhead_ = the oldest live scan
  size_t qhead_ = 0, count_ = 0;
  bool wrap_ = false;            // the newest scan lies below the oldest
};

}  // namespace vba
