// The C++ classes of the re-position search (include/lsd_slam_hip.hpp: KeyFrameBank, TrackableKeyFrameSearch, Frame::idxInKeyframes) on the
// device, against the host-cloud members they stand beside: KeyFrameBank::put / download equals Frame::setPermaRef's vectors bit for
// bit, and findRePositionCandidate over seven keyframes at one place (five of the initialisation phase, the frame's tracking parent, one
// candidate) takes the candidate.  Needs a GPU.  Usage: kfbank_classes_test   (exit status 0; prints "kfbank classes ok")
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "lsd_slam_hip.hpp"

using namespace lsd_slam_hip;

namespace {
int g_fail = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      g_fail++;                                                  \
      std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
    }                                                            \
  } while (0)
}  // namespace

int main() {
  const int w = 320, h = 240;
  const Mat3f K = Mat3f::intrinsics(170.f, 200.f, 151.f, 119.f);
  std::vector<unsigned char> img((size_t)w * h);
  std::vector<float> depth((size_t)w * h, 2.0f);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) img[(size_t)y * w + x] = (unsigned char)(128.0 + 100.0 * std::sin(0.35 * x) * std::cos(0.27 * y));
  std::shared_ptr<Context> ctx = Context::get(w, h, K);
  KeyFrameBank bank(ctx, 7);
  std::vector<std::unique_ptr<Frame>> kfs;
  const Sim3 origin;
  for (int i = 0; i < 7; i++) {
    kfs.emplace_back(new Frame(10 + i, w, h, K, 0.0, img.data()));
    Frame& kf = *kfs.back();
    kf.setDepthFromGroundTruth(depth.data());
    CHECK(kf.idxInKeyframes == -1, "fresh frame");
    CHECK(bank.put(kf, origin, 0.5f) == i && kf.idxInKeyframes == i, "slot %d", kf.idxInKeyframes);
  }
  CHECK(bank.size() == 7, "size %d", bank.size());
  // the slot's cloud is what Frame::setPermaRef keeps on the host
  TrackingReference ref;
  ref.importFrame(kfs[6].get());
  kfs[6]->setPermaRef(&ref);
  std::vector<float> pos, cv;
  const int n = bank.download(6, &pos, &cv);
  const KeyFrameBank::Info info = bank.info(6);
  CHECK(n == kfs[6]->permaRefNumPts && n > 100 && info.numPoints == n && info.frameId == 16 && info.meanIdepth == 0.5f, "%d points, %d on the host", n, kfs[6]->permaRefNumPts);
  CHECK(pos.size() == kfs[6]->permaRef_posData.size() && std::memcmp(pos.data(), kfs[6]->permaRef_posData.data(), pos.size() * 4) == 0, "pos bits");
  CHECK(cv.size() == kfs[6]->permaRef_colorAndVarData.size() && std::memcmp(cv.data(), kfs[6]->permaRef_colorAndVarData.data(), cv.size() * 4) == 0, "colorAndVar bits");
  // the search: slots 0-4 are of the initialisation phase, slot 5 is the frame's tracking parent, slot 6 is taken
  Frame frame(100, w, h, K, 0.0, img.data());
  TrackableKeyFrameSearch search(&bank, w, h, K);
  const int slot = search.findRePositionCandidate(&frame, origin, 15, 1.0f);
  const std::vector<lsdhip_reposition_record> recs = search.records();
  CHECK(slot == 6 && search.last.frameId == 16 && search.last.numPotential == 7 && search.last.numChecked == 1 && search.last.numTracked == 1,
        "slot %d potential %d checked %d tracked %d", slot, search.last.numPotential, search.last.numChecked, search.last.numTracked);
  CHECK(recs.size() == 7 && recs[0].stage == LSDHIP_REPO_INIT_PHASE && recs[5].stage == LSDHIP_REPO_PARENT && recs[6].stage == LSDHIP_REPO_TAKEN, "stages");
  CHECK(recs[6].usage == 1.0f && recs[6].score == search.getRefFrameScore(0.f, 1.f) && recs[6].poseDiscrepancy < 1e-3f && recs[6].goodVal > search.relocalizationTH,
        "usage %f score %f discrepancy %f goodVal %f", recs[6].usage, recs[6].score, recs[6].poseDiscrepancy, recs[6].goodVal);
  // the host-cloud members agree with the bank's entries for that candidate, from the search's own refToFrame (the identity)
  const SE3 T0 = SE3::from7(recs[6].refToFrame);
  CHECK(T0.q[0] == 1.0 && T0.t[0] == 0.0 && T0.t[1] == 0.0 && T0.t[2] == 0.0, "refToFrame");
  const float usage = search.tracker().checkPermaRefOverlap(kfs[6].get(), T0);
  CHECK(usage == recs[6].usage, "usage %f against %f", usage, recs[6].usage);
  const SE3 T = search.tracker().trackFrameOnPermaref(kfs[6].get(), &frame, T0);
  double p[7];
  T.to7(p);
  CHECK(std::memcmp(p, recs[6].refToFrame_tracked, sizeof(p)) == 0, "tracked pose bits: t %g %g %g against %g %g %g", p[4], p[5], p[6], recs[6].refToFrame_tracked[4],
        recs[6].refToFrame_tracked[5], recs[6].refToFrame_tracked[6]);
  CHECK(search.tracker().pointUsage == recs[6].usageTracked, "tracked usage %f against %f", search.tracker().pointUsage, recs[6].usageTracked);
  // an acceptance threshold nothing reaches: a new keyframe is to be made
  search.relocalizationTH = 1.5f;
  CHECK(search.findRePositionCandidate(&frame, origin, 15, 1.0f) == -1 && search.last.trackingBatches == 1, "nothing taken");
  // a search whose (w, h, K) name another context than the bank's says so
  bool threw = false;
  try { TrackableKeyFrameSearch other(&bank, w, h, Mat3f::intrinsics(171.f, 200.f, 151.f, 119.f)); } catch (const Error& e) { threw = e.status == LSDHIP_E_ARG; }
  CHECK(threw, "another context");
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("kfbank classes ok\n");
  return 0;
}
