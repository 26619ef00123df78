// The frame step's "late frame" rule (fusion_frame.hip, dms_fusion::late): whether the HOST waits for a frame's live half and
// enqueues the frame behind it, instead of leaving a barrier packet on the frame's queue.  Plain host code, nothing from HIP.
#pragma once

namespace dms {

struct LateFrame {
  bool on = false;  // this frame
  int forced = -1;  // DMS_LATE_MAIN: 0 / 1 forces the rule off / on
  int low = 0, cool = 0, backoff = 64;

  // Once per frame.  `may`: the context is driven alone on a map of its own (decided by the frame step); `waited_ms`: the host's
  // wait at the start of the frame (for frame t - 2) = its remaining slack.
  void update(bool may, double waited_ms) {
    if (forced >= 0) {
      on = forced != 0;
    } else if (!may) {
      on = false;
      low = 0;
    } else if (cool > 0) {
      cool -= 1;
      on = false;
    } else if (on && waited_ms < 0.015) {
      if (++low >= 3) {  // the host has no slack left: back to the barrier for a while
        on = false;
        low = 0;
        cool = backoff;
        if (backoff < 4096) backoff *= 2;
      }
    } else {
      low = 0;
      on = true;
    }
  }
};

}  // namespace dms
