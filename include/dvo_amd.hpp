/*
 * dvo_amd.hpp -- C++ host mirror of the reference's class surface for the edge-alignment path,
 * header-only on top of the C ABI (dvo_amd.h).  ROS-, OpenCV- and Eigen-free, so it builds in
 * this image; the reference's node keeps its own ROS plumbing and swaps only the bodies shown in
 * INTEGRATION.md.
 *
 *   dvo_amd::SolveDVO               include/SolveDVO.h:148-360, src/SolveDVO.cpp
 *       setCameraMatrix             :88-126   (fx,fy,cx,cy of the level-0 calibration)
 *       setRefFrame                 setRcvdFrameAsRefFrame :537-557 + preProcessRefFrame :269-303
 *                                   (selectedPts + enlistRefEdgePts run on the GPU)
 *       setNowFrame                 setRcvdFrameAsNowFrame :588-614 (the DT / gradient images of
 *                                   computeDistTransfrmOfNow :1740-1799 are the inputs)
 *       runIterations               :619-1017, same argument order and meaning
 *       alignPyramid                the level loop of SolveDVO::loop :2097-2104 (+ :2220-2227)
 *       iterationsConfig            :30-33, SolveDVO.h:354
 *       setRcvdFrame / loadFromFile imageArrivedCallBack :490-534 / loadFromFile :154-190 (OpenCV-XML mono_%d, depth_%d)
 *       setRcvdFrameAsRefFrame, setPrevFrameAsRefFrame, setRcvdFrameAsNowFrame, preProcessRefFrame
 *                                   :535-618, :269-303 -- on the engine's frame store (Canny, distance transform,
 *                                   point extraction on the GPU; the previous now frame stays resident)
 *       processFirstFrame / processFrame   the body of SolveDVO::loop :1970-2241: level schedule, forced key frame
 *                                   every 5 frames with the n-1 re-reference + re-run (__NEW__REF_UPDATE), GOP push
 *       printPose                   :1341-1354 ("qx qy qz qw tx ty tz" lines, __WRITE_EST_POSE_TO_FILE)
 *   dvo_amd::GOP<T>                 include/GOP.h, src/GOP.cpp:138-196 (key-frame relative -> global pose chain)
 *   dvo_amd::PyramidalStorageStruct include/PyramidalStorage.h:37-78 (addLevel/getLevel/clearPyramid/printSize):
 *                                   here the per-level container of the now-frame pyramid
 *   dvo_amd::RGBDOdometry           include/RGBDOdometry.h:41-43: the legacy photometric Gauss-Newton node, on the engine's
 *                                   dvo_photo_* entry points (rows A14 / f4)
 *   dvo_amd::RGBDOdometryStreams    RGBDOdometry::processFrame for K camera streams at once (dvo_photo_streams_*)
 *
 * Error behaviour: the reference asserts (NDEBUG is force-undefined, SolveDVO.h:124); these classes
 * throw std::runtime_error carrying dvo_last_error().
 */
#ifndef DVO_AMD_HPP_
#define DVO_AMD_HPP_

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "dvo_amd.h"

namespace dvo_amd {

/* Column-major float image, the layout of Eigen::MatrixXf (element (yy,xx) at yy + xx*rows). */
struct ImageF {
    int rows = 0, cols = 0;
    std::vector<float> data;
    ImageF() = default;
    ImageF(int r, int c) : rows(r), cols(c), data((size_t)r * c, 0.0f) {}
    float &operator()(int yy, int xx) { return data[(size_t)yy + (size_t)xx * rows]; }
    float operator()(int yy, int xx) const { return data[(size_t)yy + (size_t)xx * rows]; }
};
struct ImageI {
    int rows = 0, cols = 0;
    std::vector<int32_t> data;
    ImageI() = default;
    ImageI(int r, int c) : rows(r), cols(c), data((size_t)r * c, 0) {}
};

/* cv::Mat / Eigen stand-ins of the legacy photometric path (row-major 8/16-bit images like cv::Mat; column-major double
 * arrays like Eigen::ArrayXXd / MatrixXd) */
struct ImageU8 { int rows = 0, cols = 0, channels = 1; std::vector<unsigned char> data; };      /* CV_8UC1 / CV_8UC3 */
struct ImageU16 { int rows = 0, cols = 0; std::vector<unsigned short> data; };                  /* CV_16UC1 */
struct ArrayD { int rows = 0, cols = 0; std::vector<double> data; };                            /* Eigen::ArrayXXd / MatrixXd */

/* include/PyramidalStorage.h:37-78.  Two uses:
 *  - the reference's own 11-field per-level record of the photometric estimators (im_r_color, im_r, dim_r, X, Y, Z, J,
 *    grayVals, redVals, greenVals, blueVals): addLevel pushes deep copies and ignores its level argument
 *    (PyramidalStorage.cpp:37-65), getLevel copies them back out (:71-102), clearPyramid, printSize (:105-127);
 *  - the 3-image form {DT, dDT/dx, dDT/dy} SolveDVO::setNowFrame of this header takes (SolveDVO itself keeps
 *    std::vector<Eigen::MatrixXf> members; the container shape is kept for both). */
class PyramidalStorageStruct {
public:
    void addLevel(int /*level: ignored, PyramidalStorage.cpp:37*/, const ImageU8 &im_r_color, const ImageU8 &im_r, const ImageU16 &dim_r,
                  const ArrayD &X, const ArrayD &Y, const ArrayD &Z, const ArrayD &J,
                  const ArrayD &grayVals, const ArrayD &redVals, const ArrayD &greenVals, const ArrayD &blueVals) {
        im_r_color_.push_back(im_r_color); im_r_.push_back(im_r); dim_r_.push_back(dim_r);
        X_.push_back(X); Y_.push_back(Y); Z_.push_back(Z); J_.push_back(J);
        gray_.push_back(grayVals); red_.push_back(redVals); green_.push_back(greenVals); blue_.push_back(blueVals);
    }
    void getLevel(int level, ImageU8 &im_r_color, ImageU8 &im_r, ImageU16 &dim_r, ArrayD &X, ArrayD &Y, ArrayD &Z, ArrayD &J,
                  ArrayD &grayVals, ArrayD &redVals, ArrayD &greenVals, ArrayD &blueVals) const {
        im_r_color = im_r_color_.at(level); im_r = im_r_.at(level); dim_r = dim_r_.at(level);         /* deep copies, :85-99 */
        X = X_.at(level); Y = Y_.at(level); Z = Z_.at(level); J = J_.at(level);
        grayVals = gray_.at(level); redVals = red_.at(level); greenVals = green_.at(level); blueVals = blue_.at(level);
    }
    void addLevel(int /*level*/, const ImageF &dt, const ImageF &gx, const ImageF &gy) { dt_.push_back(dt); gx_.push_back(gx); gy_.push_back(gy); }
    void getLevel(int level, ImageF &dt, ImageF &gx, ImageF &gy) const { dt = dt_.at(level); gx = gx_.at(level); gy = gy_.at(level); }
    void clearPyramid() {
        dt_.clear(); gx_.clear(); gy_.clear();
        im_r_color_.clear(); im_r_.clear(); dim_r_.clear(); X_.clear(); Y_.clear(); Z_.clear(); J_.clear();
        gray_.clear(); red_.clear(); green_.clear(); blue_.clear();
    }
    void printSize() const {                            /* PyramidalStorage.cpp:125-127 prints the vector sizes */
        std::printf("PyramidalStorageStruct: %zu DT levels, %zu photometric levels\n", dt_.size(), im_r_.size());
    }
    size_t size() const { return dt_.size(); }
    size_t photometricLevels() const { return im_r_.size(); }
private:
    std::vector<ImageF> dt_, gx_, gy_;
    std::vector<ImageU8> im_r_color_, im_r_;
    std::vector<ImageU16> dim_r_;
    std::vector<ArrayD> X_, Y_, Z_, J_, gray_, red_, green_, blue_;
};

/* geometry_msgs::Pose stand-in */
struct Pose { double px = 0, py = 0, pz = 0, qx = 0, qy = 0, qz = 0, qw = 1; };

/* Eigen::Quaternion<T>(Matrix3) as GOPElement::matrixToPose uses it (src/GOP.cpp:103-115); R column-major */
template <typename T>
inline void quaternionFromMatrix(const T *R, T &qx, T &qy, T &qz, T &qw) {
    auto m = [&](int i, int j) { return R[i + 3 * j]; };
    T t = m(0, 0) + m(1, 1) + m(2, 2);
    if (t > T(0)) {
        t = std::sqrt(t + T(1.0));
        qw = T(0.5) * t;
        t = T(0.5) / t;
        qx = (m(2, 1) - m(1, 2)) * t; qy = (m(0, 2) - m(2, 0)) * t; qz = (m(1, 0) - m(0, 1)) * t;
    } else {
        int i = 0;
        if (m(1, 1) > m(0, 0)) i = 1;
        if (m(2, 2) > m(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + T(1.0));
        T q[3];
        q[i] = T(0.5) * t;
        t = T(0.5) / t;
        qw = (m(k, j) - m(j, k)) * t;
        q[j] = (m(j, i) + m(i, j)) * t;
        q[k] = (m(k, i) + m(i, k)) * t;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
}

/* Key-frame relative poses -> global pose chain (include/GOP.h, src/GOP.cpp:138-196). */
template <typename T>
class GOP {
public:
    struct Element { int frameNum; bool keyFrame; int reason; T R[9]; T t[3]; };
    GOP() { identity(lastKeyFr_R_); lastKeyFr_T_[0] = lastKeyFr_T_[1] = lastKeyFr_T_[2] = T(0); }
    void pushAsOrdinaryFrame(int frameNum, const T *cR, const T *cT) {            /* GOP.cpp:138-153 */
        Element e; compose(cR, cT, e.R, e.t);
        e.frameNum = frameNum; e.keyFrame = false; e.reason = -1;
        v_.push_back(e);
    }
    void pushAsKeyFrame(int frameNum, int reason, const T *cR, const T *cT) {      /* GOP.cpp:162-186 */
        Element e; compose(cR, cT, e.R, e.t);
        e.frameNum = frameNum; e.keyFrame = true; e.reason = reason;
        v_.push_back(e);
        for (int k = 0; k < 9; k++) lastKeyFr_R_[k] = e.R[k];
        for (int k = 0; k < 3; k++) lastKeyFr_T_[k] = e.t[k];
    }
    void updateMostRecentToKeyFrame(int reason) {                                  /* GOP.cpp:189-196 */
        Element &e = v_.at(v_.size() - 1);
        for (int k = 0; k < 9; k++) lastKeyFr_R_[k] = e.R[k];
        for (int k = 0; k < 3; k++) lastKeyFr_T_[k] = e.t[k];
        e.keyFrame = true; e.reason = reason;
    }
    int size() const { return (int)v_.size(); }
    const T *getGlobalRAt(int i) const { return v_.at(i).R; }
    const T *getGlobalTAt(int i) const { return v_.at(i).t; }
    bool isKeyFrameAt(int i) const { return v_.at(i).keyFrame; }
    int getReasonAt(int i) const { return v_.at(i).reason; }
    int getFrameNumAt(int i) const { return v_.at(i).frameNum; }
    Pose getGlobalPoseAt(int i) const {
        const Element &e = v_.at(i);
        Pose p; T qx, qy, qz, qw;
        quaternionFromMatrix<T>(e.R, qx, qy, qz, qw);
        p.px = e.t[0]; p.py = e.t[1]; p.pz = e.t[2]; p.qx = qx; p.qy = qy; p.qz = qz; p.qw = qw;
        return p;
    }
private:
    static void identity(T *R) { for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? T(1) : T(0); }
    void compose(const T *cR, const T *cT, T *gR, T *gT) const {   /* global_T = key_T + key_R*cT; global_R = key_R*cR */
        for (int i = 0; i < 3; i++) {
            gT[i] = lastKeyFr_T_[i] + (lastKeyFr_R_[i] * cT[0] + lastKeyFr_R_[i + 3] * cT[1] + lastKeyFr_R_[i + 6] * cT[2]);
            for (int j = 0; j < 3; j++)
                gR[i + 3 * j] = lastKeyFr_R_[i] * cR[3 * j] + lastKeyFr_R_[i + 3] * cR[3 * j + 1] + lastKeyFr_R_[i + 6] * cR[3 * j + 2];
        }
    }
    std::vector<Element> v_;
    T lastKeyFr_R_[9], lastKeyFr_T_[3];
};

/* One received frame: the pyramid of the RGBDFramePyd message (msg/RGBDFramePyd.msg: framemono[] mono8, dframe[]
 * mono16), row-major like cv::Mat / sensor_msgs::Image. */
struct RGBDFramePyd {
    struct Level { int rows = 0, cols = 0; std::vector<uint8_t> mono; std::vector<uint16_t> depth; };
    std::vector<Level> levels;
};

/* OpenCV FileStorage XML written by the publisher (camTopic2PublisherPyD.cpp:306-383): matrices mono_%d (dt u) and
 * depth_%d (dt w).  Minimal reader for that layout: <name type_id="opencv-matrix"><rows><cols><dt><data>. */
inline bool readOpenCvXmlMatrix(const std::string &xml, const std::string &name, int &rows, int &cols, std::string &dt,
                                std::vector<double> &values) {
    size_t a = xml.find("<" + name + " ");
    if (a == std::string::npos) a = xml.find("<" + name + ">");
    if (a == std::string::npos) return false;
    const size_t end = xml.find("</" + name + ">", a);
    auto field = [&](const char *tag, std::string &out) {
        const std::string open = std::string("<") + tag + ">", close = std::string("</") + tag + ">";
        const size_t b = xml.find(open, a);
        if (b == std::string::npos || b > end) return false;
        const size_t e = xml.find(close, b);
        if (e == std::string::npos) return false;
        out = xml.substr(b + open.size(), e - b - open.size());
        return true;
    };
    std::string r, c, d;
    if (!field("rows", r) || !field("cols", c) || !field("dt", dt) || !field("data", d)) return false;
    rows = std::atoi(r.c_str()); cols = std::atoi(c.c_str());
    while (!dt.empty() && (dt.back() == ' ' || dt.back() == '\n')) dt.pop_back();
    while (!dt.empty() && (dt.front() == ' ' || dt.front() == '\n')) dt.erase(dt.begin());
    values.clear();
    values.reserve((size_t)rows * cols);
    const char *p = d.c_str();
    char *q = nullptr;
    for (;;) {
        const double v = std::strtod(p, &q);
        if (q == p) break;
        values.push_back(v);
        p = q;
    }
    return (int)values.size() == rows * cols;
}

/* minimal reader for the <cameraMatrix> ... <data> fx 0 cx 0 fy cy 0 0 1 </data> node of an OpenCV calibration XML
 * (SolveDVO::setCameraMatrix(const char*), SolveDVO.cpp:88-126): the 9 entries of K, row-major */
inline void readCameraMatrix(const char *calibFile, double k[9]) {
    std::FILE *f = std::fopen(calibFile, "r");
    if (!f) throw std::runtime_error(std::string("Cannot open calibration file ") + calibFile);   /* ROS_ERROR at :94-99 */
    std::string s; char buf[4096]; size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
    std::fclose(f);
    size_t a = s.find("cameraMatrix");
    a = (a == std::string::npos) ? a : s.find("<data>", a);
    if (a == std::string::npos) throw std::runtime_error("cameraMatrix/data node not found");
    if (std::sscanf(s.c_str() + a + 6, "%lf %lf %lf %lf %lf %lf %lf %lf %lf", k, k + 1, k + 2, k + 3, k + 4, k + 5, k + 6, k + 7, k + 8) != 9)
        throw std::runtime_error("cameraMatrix/data: expected 9 numbers");
}

class SolveDVO {
public:
    std::vector<int> iterationsConfig;      /* SolveDVO.cpp:30-33 */
    GOP<double> gop;                        /* SolveDVO.h: GOP<double> gop */

    explicit SolveDVO(const dvo_params *params = nullptr) {
        iterationsConfig = {50, 50, 50, 50};
        if (dvo_create(params, &ctx_) != DVO_OK) throw std::runtime_error(std::string("dvo_create: ") + dvo_last_error(nullptr));
    }
    ~SolveDVO() { dvo_destroy(ctx_); }
    SolveDVO(const SolveDVO &) = delete;
    SolveDVO &operator=(const SolveDVO &) = delete;

    /* SolveDVO::setCameraMatrix(const char*) reads an OpenCV calibration XML (SolveDVO.cpp:88-126); the
     * numbers it keeps are these four (fx, fy, cx, cy of K, SolveDVO.h:178-179). */
    void setCameraMatrix(float fx, float fy, float cx, float cy) { chk(dvo_set_intrinsics(ctx_, fx, fy, cx, cy)); isCameraIntrinsicsAvailable = true; }
    void setCameraMatrix(const char *calibFile) {
        double k[9];
        readCameraMatrix(calibFile, k);
        setCameraMatrix((float)k[0], (float)k[4], (float)k[2], (float)k[5]);
    }

    /* reference frame: per level an edge map (>0 = edge) and a depth image in mm; the 3-D edge point
     * lists _ref_edge_3d/_ref_edge_2d are built on the GPU (preProcessRefFrame :269-303). */
    void setRefFrame(const std::vector<ImageI> &edge, const std::vector<ImageF> &depth_mm) {
        if (edge.size() != depth_mm.size()) throw std::runtime_error("edge/depth pyramids differ in size");
        ref_points_.assign(edge.size(), {});
        for (size_t l = 0; l < edge.size(); l++) {
            const int cap = edge[l].rows * edge[l].cols;
            std::vector<float> xyz((size_t)3 * cap);
            int N = 0;
            chk(dvo_set_ref_level_from_images(ctx_, 0, (int)l, edge[l].data.data(), depth_mm[l].data.data(),
                                              edge[l].rows, edge[l].cols, xyz.data(), nullptr, cap, &N));
            xyz.resize((size_t)3 * N);
            ref_points_[l] = xyz;
        }
        isRefFrameAvailable = true;
    }
    /* or directly the 3 x N lists (SpaceCordList, SolveDVO.h:137,304) */
    void setRefEdgePoints(int level, const float *xyz_3xN, int N) {
        chk(dvo_set_ref_level(ctx_, level, xyz_3xN, N));
        if ((int)ref_points_.size() <= level) ref_points_.resize(level + 1);
        ref_points_[level].assign(xyz_3xN, xyz_3xN + (size_t)3 * N);
        isRefFrameAvailable = true;
    }
    /* now frame: now_distance_transform / now_DT_gradientX / now_DT_gradientY of every level */
    void setNowFrame(const PyramidalStorageStruct &pyr) {
        for (size_t l = 0; l < pyr.size(); l++) {
            ImageF dt, gx, gy;
            pyr.getLevel((int)l, dt, gx, gy);
            chk(dvo_set_now_level(ctx_, (int)l, dt.data.data(), gx.data.data(), gy.data.data(), dt.rows, dt.cols));
        }
        isNowFrameAvailable = true;
    }

    /* SolveDVO::runIterations (SolveDVO.h:228-230): cR 3x3 column-major, cT 3, both in/out. */
    void runIterations(int level, int maxIterations, double *cR, double *cT,
                       std::vector<float> &energyAtEachIteration, std::vector<float> &finalEpsilons,
                       std::vector<float> &finalReprojections, int &bestEnergyIndex, float &finalVisibleRatio) {
        if (!(isRefFrameAvailable && isNowFrameAvailable && isCameraIntrinsicsAvailable))          /* :627 */
            throw std::runtime_error("runIterations: reference frame, now frame and intrinsics must be set");
        const size_t N = ref_points_.at(level).size() / 3;
        energyAtEachIteration.assign(maxIterations, 0.0f);                                          /* :634 */
        finalEpsilons.assign(N, 0.0f);
        finalReprojections.assign(3 * N, 0.0f);
        chk(dvo_run_iterations(ctx_, level, maxIterations, cR, cT, energyAtEachIteration.data(),
                               finalEpsilons.data(), finalReprojections.data(), &bestEnergyIndex, &finalVisibleRatio));
    }

    /* the level loop of SolveDVO::loop (:2097-2104): for f = size-1 .. 0: if cfg[f] > 0: runIterations(f, ...) --
     * fused into one kernel launch. */
    void alignPyramid(double *cR, double *cT, int flags = 0) {
        chk(dvo_align_pyramid(ctx_, (int)iterationsConfig.size(), iterationsConfig.data(), flags, cR, cT));
    }
    /* processResidueHistogram (:1398-1481) without its display: the MLE of the Laplacian scale of the residues = their mean,
     * accumulated in float in the list's order as the reference does (:1455-1462) */
    static float processResidueHistogram(const std::vector<float> &residi) {
        float b_cap = 0;
        for (size_t i = 0; i < residi.size(); i++) b_cap += residi[i];
        return residi.empty() ? 0.0f : b_cap / (float)residi.size();
    }
    void levelReport(int level, std::vector<float> &energy, int &bestEnergyIndex, float &visibleRatio) {
        energy.assign(iterationsConfig.at(level), 0.0f);
        chk(dvo_get_level_report(ctx_, 0, level, energy.data(), (int)energy.size(), &bestEnergyIndex, &visibleRatio));
    }

    /* ---- frames in: the engine's frame store instead of host copies + OpenCV -------------------------------- */
    /* the camera's ignore mask (dvo_frames_set_pair_mask for pair 0): rows x cols bytes at the camera's resolution, non-zero = "not the
     * world"; the received pyramids must be that image decimated by 2^(firstShift + l), l < nLevels (the reference publishes 4 levels
     * from firstShift 1).  NULL removes it.  margin: dilation in level pixels, 2 covers Canny's support.  From the next received frame
     * on, edge maps only.  While a mask is set, setRcvdFrame already makes the frame the engine's now level */
    void setMask(const unsigned char *mask, int rows, int cols, int nLevels = 4, int firstShift = 1, int margin = 2) {
        chk(dvo_frames_set_pair_mask(ctx_, 0, rows, cols, mask, nLevels, firstShift, margin));
        hasMask_ = mask != nullptr;
    }
    /* imageArrivedCallBack (:490-534): hand the received pyramid to the engine (upload + Canny per level) */
    void setRcvdFrame(const RGBDFramePyd &f) {
        std::vector<dvo_image> g(f.levels.size()), d(f.levels.size());
        for (size_t l = 0; l < f.levels.size(); l++) {
            const RGBDFramePyd::Level &L = f.levels[l];
            g[l] = dvo_image{L.mono.data(), L.rows, L.cols, DVO_PIX_U8, DVO_LAYOUT_ROW_MAJOR};
            d[l] = dvo_image{L.depth.data(), L.rows, L.cols, DVO_PIX_U16, DVO_LAYOUT_ROW_MAJOR};
        }
        rcvd_slot_ = freeSlot();
        /* with a mask the frame goes up as pair 0's now frame: that is what the mask applies to (setRcvdFrameAsNowFrame installs it again) */
        chk(dvo_frames_upload_pyramids(ctx_, rcvd_slot_, 1, (int)f.levels.size(), g.data(), d.data(), hasMask_ ? 0 : -1, 0));
        isFrameAvailable = true;
    }
    /* loadFromFile (:154-190): mono_0..3 / depth_0..3 of an OpenCV-XML frame file; false if it cannot be read */
    bool loadFromFile(const char *xmlFileName, int nLevels = 4) {
        std::FILE *fp = std::fopen(xmlFileName, "rb");
        if (!fp) return false;                                                     /* ROS_ERROR "Cannot Open File" :160 */
        /* The loader's buffers are members and keep their capacity from frame to frame.  Not a nicety: a host process that
         * frees multi-megabyte blocks between frames (free -> munmap) was measured to stall its own GPU queues for 14-33 ms per
         * frame on this pool (profiles/r03_single_stream: 24 ms instead of 0.6 ms per tracked frame, intermittently per
         * process; gone with glibc told never to return memory, MALLOC_MMAP_THRESHOLD_ / MALLOC_TRIM_THRESHOLD_). */
        std::string &s = loadText_; char buf[1 << 16]; size_t n;
        s.clear();
        while ((n = std::fread(buf, 1, sizeof(buf), fp)) > 0) s.append(buf, n);
        std::fclose(fp);
        RGBDFramePyd &f = loadFrame_;
        f.levels.resize(nLevels);
        std::vector<double> &v = loadV_, &w = loadW_;
        for (int i = 0; i < nLevels; i++) {
            int r = 0, c = 0, r2 = 0, c2 = 0; std::string dt;
            if (!readOpenCvXmlMatrix(s, "mono_" + std::to_string(i), r, c, dt, v)) return false;
            if (!readOpenCvXmlMatrix(s, "depth_" + std::to_string(i), r2, c2, dt, w) || r2 != r || c2 != c) return false;
            RGBDFramePyd::Level &L = f.levels[i];
            L.rows = r; L.cols = c;
            L.mono.assign(v.begin(), v.end());
            L.depth.assign(w.begin(), w.end());
        }
        setRcvdFrame(f);
        return true;
    }
    void setRcvdFrameAsRefFrame() {                 /* :535-556 (+ computeDistTransfrmOfRef: the Canny edge map is already resident) */
        need(isFrameAvailable, "setRcvdFrameAsRefFrame: no frame received");
        ref_slot_ = rcvd_slot_;
        isRefFrameAvailable = false; refPreprocessed_ = false;
    }
    void setPrevFrameAsRefFrame() {                 /* :559-583: the previous now frame is still in the store */
        need(prev_slot_ >= 0, "setPrevFrameAsRefFrame: n-1 frame not available");
        ref_slot_ = prev_slot_;
        isRefFrameAvailable = false; refPreprocessed_ = false;
    }
    void preProcessRefFrame() {                     /* :269-303: selectedPts + enlistRefEdgePts per level */
        need(ref_slot_ >= 0, "preProcessRefFrame: no reference frame");
        const int nl = dvo_frames_num_levels(ctx_);
        std::vector<int> N(nl);
        chk(dvo_frames_as_ref(ctx_, ref_slot_, 0, 1, N.data()));
        ref_points_.resize(nl);                      /* keep the capacity (see loadFromFile) */
        for (int l = 0; l < nl; l++) {
            ref_points_[l].resize((size_t)3 * N[l]);
            int n = 0;
            chk(dvo_get_ref_level(ctx_, 0, l, ref_points_[l].data(), N[l], &n));
        }
        isRefFrameAvailable = true; refPreprocessed_ = true;
    }
    void setRcvdFrameAsNowFrame() {                 /* :587-618 incl. computeDistTransfrmOfNow :1740-1799 */
        need(isFrameAvailable, "setRcvdFrameAsNowFrame: FRAME NOT AVAILABLE");
        if (isNowFrameAvailable && now_slot_ >= 0) prev_slot_ = now_slot_;         /* p_now_framemono / p_now_depth :594-600 */
        now_slot_ = rcvd_slot_;
        chk(dvo_frames_as_now(ctx_, now_slot_, 0, 1));
        isNowFrameAvailable = true;
    }

    /* ---- the body of SolveDVO::loop (:1970-2241), one call per received frame ------------------------------------ */
    /* first frame: reference frame + first key frame (:1972-2021) */
    void processFirstFrame() {
        setRcvdFrameAsRefFrame();
        preProcessRefFrame();
        if (warmUpOnFirstFrame) {
            /* one throw-away alignment of the first frame against itself: the first alignment of a process pays for loading the
             * kernels' code objects and for the engine's lazily allocated buffers (measured 12.5 ms against 0.6 ms for every later
             * frame, profiles/r03_single_stream) -- paid here, where the reference's loop has no pose to deliver yet (:1972-2021),
             * instead of on the first tracked frame.  Nothing of it survives: the now level is rewritten by the next frame. */
            chk(dvo_frames_as_now(ctx_, ref_slot_, 0, 1));
            double wR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, wT[3] = {0, 0, 0};
            alignPyramid(wR, wT);
        }
        lastRefFrame = 0;
        identityPose();
        gop.pushAsKeyFrame((int)nFrame, 1, cR_64, cT_64);
        isFrameAvailable = false;
        nFrame++;
    }
    /* every other frame (:2059-2241 with __NEW__REF_UPDATE): returns the latest global pose (what publishGOP hands to printPose) */
    Pose processFrame() {
        const auto t0 = std::chrono::steady_clock::now();
        setRcvdFrameAsNowFrame();
        if (syncAfterNowFrame) chk(dvo_synchronize(ctx_));                          /* diagnostics: separates the two stages' times */
        const auto t1 = std::chrono::steady_clock::now();
        alignPyramid(cR_64, cT_64, adaptiveKeyFrames ? DVO_FLAG_FINAL_OUTPUTS : 0);  /* :2097-2104 (warm start from the last estimate) */
        const auto t2 = std::chrono::steady_clock::now();
        lastNowFrameMs = std::chrono::duration<double, std::milli>(t1 - t0).count();
        lastAlignMs = std::chrono::duration<double, std::milli>(t2 - t1).count();   /* jdur of :2092-2109 */
        bool signalGetNewRefImage = false;
        int reasonForChange = 0;
        if (adaptiveKeyFrames) {
            /* the three exits the reference has commented out (:2129-2152), evaluated on the last level that ran -- its best iterate's
             * visible ratio, finalEpsilons and point count, as the loop leaves them (:2102).  As written there the statement that
             * follows them (`signalGetNewRefImage = false`, :2154) would void all three; here they are OR-ed with the live rule. */
            int last = -1;
            for (int f = 0; f < (int)iterationsConfig.size() && last < 0; f++) if (iterationsConfig[f] > 0) last = f;
            need(last >= 0, "processFrame: no level has iterations");
            std::vector<float> energy; int best = -1; float visibleRatio = 1.0f;
            levelReport(last, energy, best, visibleRatio);
            int n = 0;
            epsilonVec_.assign(ref_points_.at(last).size() / 3, 0.0f);              /* one residue per reference point of that level */
            chk(dvo_get_final_outputs(ctx_, 0, epsilonVec_.data(), nullptr, (int)epsilonVec_.size(), &n));
            epsilonVec_.resize((size_t)n);
            lastLaplacianB = processResidueHistogram(epsilonVec_);                  /* b_cap :2116-2120 */
            lastVisibleRatio = visibleRatio;
            lastNumPoints = n;
            if (lastLaplacianB > laplacianThreshExitCond) { signalGetNewRefImage = true; reasonForChange = 2; }      /* :2131-2136 */
            if (visibleRatio < ratio_of_visible_pts_thresh) { signalGetNewRefImage = true; reasonForChange = 3; }    /* :2139-2144 */
            if (n < minReprojectedPoints) { signalGetNewRefImage = true; reasonForChange = 4; }                      /* :2146-2151 */
        }
        if ((nFrame - lastRefFrame) == keyFrameEvery) { signalGetNewRefImage = true; reasonForChange = 5; }   /* :2155-2160 */
        if (signalGetNewRefImage && lastRefFrame != nFrame - 1) {                  /* :2198 */
            lastRefFrame = nFrame - 1;
            setPrevFrameAsRefFrame();
            preProcessRefFrame();
            gop.updateMostRecentToKeyFrame(reasonForChange);                       /* :2207 */
            identityPose();                                                        /* :2210-2211 */
            alignPyramid(cR_64, cT_64);                                            /* re-run :2220-2227 */
            gop.pushAsOrdinaryFrame((int)nFrame, cR_64, cT_64);                    /* :2232 */
        } else {
            gop.pushAsOrdinaryFrame((int)nFrame, cR_64, cT_64);                    /* :2239 */
        }
        isFrameAvailable = false;
        nFrame++;
        return gop.getGlobalPoseAt(gop.size() - 1);                                /* MentisVisualHandle::publishGOP :283-300 */
    }
    /* printPose (:1341-1354): the line format of poses/estPoses.txt */
    static void printPose(const Pose &p, std::ostream &stream) {
        stream << p.qx << " " << p.qy << " " << p.qz << " " << p.qw << " " << p.px << " " << p.py << " " << p.pz << "\n";
        stream.flush();
    }
    double lastNowFrameMs = 0, lastAlignMs = 0;                                    /* iterationsComputeTime of :2107 and its preprocessing */
    double cR_64[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, cT_64[3] = {0, 0, 0};          /* key-frame relative estimate (column-major) */
    long nFrame = 0, lastRefFrame = 0;
    int keyFrameEvery = 5;                                                         /* (nFrame - lastRefFrame) == 5  :2156 */
    /* the reference's adaptive key-frame signals (:2129-2152, commented out there; constants :22-23): off by default */
    bool adaptiveKeyFrames = false;
    float ratio_of_visible_pts_thresh = 0.8f, laplacianThreshExitCond = 3.0f;
    int minReprojectedPoints = 50;
    float lastLaplacianB = 0.0f, lastVisibleRatio = 1.0f;                          /* what the last frame's first alignment produced */
    int lastNumPoints = 0;

    /* casualTestFunction (:2377-2442), the reference's only two-frame regression of the hot path: frame `refFile` as the
     * reference frame, `nowFile` as the now frame (TUM_RGBD/fr1_rpy/framemono_0080.xml and _0085.xml there, not shipped),
     * runIterations(0, 100, ...) from the identity (:2426); returns the 100 energies it prints (:2438-2441) */
    std::vector<float> casualTestFunction(const char *refFile, const char *nowFile, int level = 0, int iterations = 100,
                                          bool print = true) {
        const int nl = (int)iterationsConfig.size();        /* levels per frame file (4 in the reference) */
        need(loadFromFile(refFile, nl), "casualTestFunction: cannot read the reference frame file");
        setRcvdFrameAsRefFrame();
        preProcessRefFrame();
        need(loadFromFile(nowFile, nl), "casualTestFunction: cannot read the now frame file");
        setRcvdFrameAsNowFrame();
        identityPose();
        std::vector<float> energy, eps, reproj;
        int best = -1; float ratio = 0;
        runIterations(level, iterations, cR_64, cT_64, energy, eps, reproj, best, ratio);
        if (print) {
            for (size_t i = 0; i < energy.size(); i++) std::printf("%zu: %f\n", i, energy[i]);
            std::printf("best %d, visible ratio %f\n", best, ratio);
        }
        return energy;
    }

    /* frame loop hooks of the reference; the ROS node keeps its own loop() */
    void loopDry() {}
    void loopFromFile() { throw std::runtime_error("loopFromFile: body is commented out in the reference too (SolveDVO.cpp:2444-2678)"); }

    dvo_ctx *handle() { return ctx_; }

private:
    std::vector<float> epsilonVec_;                                                /* keeps its capacity from frame to frame */
    void chk(int rc) { if (rc != DVO_OK) throw std::runtime_error(dvo_last_error(ctx_)); }
    static void need(bool ok, const char *what) { if (!ok) throw std::runtime_error(what); }
public:
    bool warmUpOnFirstFrame = true;                 /* see processFirstFrame */
    bool syncAfterNowFrame = false;                 /* diagnostics (tools/track_latency.py): wait for the now-frame stage before timing the alignment */
private:
    void identityPose() { for (int k = 0; k < 9; k++) cR_64[k] = (k % 4 == 0) ? 1.0 : 0.0; cT_64[0] = cT_64[1] = cT_64[2] = 0.0; }
    int freeSlot() const {                          /* a store slot that holds neither the reference, the now nor the n-1 frame */
        for (int s = 0; s < 4; s++) if (s != ref_slot_ && s != now_slot_ && s != prev_slot_) return s;
        return 3;
    }
    dvo_ctx *ctx_ = nullptr;
    std::string loadText_;                          /* loadFromFile: reused from frame to frame */
    std::vector<double> loadV_, loadW_;
    RGBDFramePyd loadFrame_;
    std::vector<std::vector<float>> ref_points_;
    bool isCameraIntrinsicsAvailable = false, isRefFrameAvailable = false, isNowFrameAvailable = false;
    bool isFrameAvailable = false, refPreprocessed_ = false, hasMask_ = false;
    int rcvd_slot_ = -1, ref_slot_ = -1, now_slot_ = -1, prev_slot_ = -1;
};

/* OpenCV-XML frame file (mono_0.. / depth_0.., loadFromFile :154-190) -> f; false if it cannot be read.  text / v / w are the caller's
 * buffers, kept from frame to frame (see SolveDVO::loadFromFile) */
inline bool loadFrameXml(const char *xmlFileName, int nLevels, RGBDFramePyd &f, std::string &text, std::vector<double> &v,
                         std::vector<double> &w) {
    std::FILE *fp = std::fopen(xmlFileName, "rb");
    if (!fp) return false;
    char buf[1 << 16]; size_t n;
    text.clear();
    while ((n = std::fread(buf, 1, sizeof(buf), fp)) > 0) text.append(buf, n);
    std::fclose(fp);
    f.levels.resize(nLevels);
    for (int i = 0; i < nLevels; i++) {
        int r = 0, c = 0, r2 = 0, c2 = 0; std::string dt;
        if (!readOpenCvXmlMatrix(text, "mono_" + std::to_string(i), r, c, dt, v)) return false;
        if (!readOpenCvXmlMatrix(text, "depth_" + std::to_string(i), r2, c2, dt, w) || r2 != r || c2 != c) return false;
        RGBDFramePyd::Level &L = f.levels[i];
        L.rows = r; L.cols = c;
        L.mono.assign(v.begin(), v.end());
        L.depth.assign(w.begin(), w.end());
    }
    return true;
}

/* Covariance of a pose from the tracker's information record (dvo_tracker_get_information): C = s^2 H^-1 with the residual variance
 * s^2 = sum_eps2 / (n_visible - 6), H^-1 by Cholesky in double; H36 and C36 are symmetric 6x6 matrices in the component order
 * [translation x, y, z, rotation x, y, z].  What it is: the Gauss-Newton approximation with the robust weights held fixed, in the units
 * of the distance-transform residual -- a relative, uncalibrated scale that a consumer may rescale (e.g. against a ground-truth
 * segment).  Returns false and leaves C36 alone when n_visible <= 6 or H is not positive definite.  Host only.
 * (rgbd_odometry_amd.capi.pose_covariance is the same formula.) */
inline bool poseCovariance(const double H36[36], double sum_eps2, int n_visible, double C36[36]) {
    if (n_visible <= 6) return false;
    double L[36] = {0}, Li[36] = {0};
    for (int k = 0; k < 36; k++) if (!std::isfinite(H36[k])) return false;
    for (int j = 0; j < 6; j++) {                    /* H = L L^T */
        double d = H36[j * 6 + j];
        for (int k = 0; k < j; k++) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0.0)) return false;
        L[j * 6 + j] = std::sqrt(d);
        for (int i = j + 1; i < 6; i++) {
            double v = H36[i * 6 + j];
            for (int k = 0; k < j; k++) v -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = v / L[j * 6 + j];
        }
    }
    for (int k = 0; k < 6; k++)                      /* L^-1 by forward substitution */
        for (int i = k; i < 6; i++) {
            double v = (i == k) ? 1.0 : 0.0;
            for (int m = k; m < i; m++) v -= L[i * 6 + m] * Li[m * 6 + k];
            Li[i * 6 + k] = v / L[i * 6 + i];
        }
    const double s2 = sum_eps2 / (double)(n_visible - 6);
    for (int i = 0; i < 6; i++)                      /* H^-1 = L^-T L^-1 */
        for (int j = 0; j < 6; j++) {
            double v = 0.0;
            for (int m = 0; m < 6; m++) v += Li[m * 6 + i] * Li[m * 6 + j];
            C36[i * 6 + j] = s2 * v;
        }
    return true;
}

/* Entry i (0 .. 63, clamped) of the jet map the tracker's residue heat map is coloured with (FColorMap), from its closed form, for
 * hosts that draw their own legend: {B, G, R} */
inline std::array<unsigned char, 3> jetColour(int i) {
    auto r = [](int j) { return j <= 0 ? 0 : std::min(255, 16 * j - 1); };
    i = std::max(0, std::min(63, i));
    return {(unsigned char)std::min(r(i + 9), r(39 - i)), (unsigned char)std::min(r(i - 7), r(55 - i)),
            (unsigned char)std::min(r(i - 23), r(71 - i))};
}

/* Whether a record of dvo_tracker_verify (SolveDVOStreams::verifyKeyFrames) supports its candidate: enough points with a depth
 * measurement, enough of those agreeing with it, few enough in front of the measured surface (free-space violations; points behind it
 * are occlusions and neutral).  Pure host arithmetic; the thresholds are the caller's (0.8, 0.05 and a few hundred points are usual) */
inline bool depthVerdict(const dvo_tracker_verify_record &r, double min_agree_ratio, double max_front_ratio, int min_depth_points) {
    return r.n_depth >= min_depth_points && (double)r.n_agree >= min_agree_ratio * (double)r.n_depth &&
           (double)r.n_front <= max_front_ratio * (double)r.n_depth;
}

/* Many camera streams in one process (dvo_tracker_*, include/dvo_amd.h): K independent copies of SolveDVO's loop (:1970-2241),
 * advanced together.  Per stream the same key-frame policy, relative poses and GOP<double> chain as SolveDVO::processFirstFrame /
 * processFrame produce for that stream's frames alone; the engine runs each stage once per tick for all listed streams. */
class SolveDVOStreams {
public:
    std::vector<GOP<double>> gop;                   /* one pose chain per stream (SolveDVO::gop) */
    std::vector<int> lastEvents;                    /* of the last processFrames call, per listed stream: 0 ordinary, 1 first frame,
                                                       2..5 reasonForChange of a key-frame switch */

    /* tp: NULL = dvo_tracker_params_default (640x480 camera frames, 4 levels from 320x240, 50 iterations per level) */
    explicit SolveDVOStreams(int maxStreams, const dvo_tracker_params *tp = nullptr, const dvo_params *params = nullptr)
        : gop(maxStreams), nFrame_(maxStreams, 0) {
        if (tp) tp_ = *tp; else dvo_tracker_params_default(&tp_);
        if (dvo_tracker_create(params, maxStreams, &tp_, &tr_) != DVO_OK)
            throw std::runtime_error(std::string("dvo_tracker_create: ") + dvo_tracker_last_error(nullptr));
    }
    ~SolveDVOStreams() { dvo_tracker_destroy(tr_); }
    SolveDVOStreams(const SolveDVOStreams &) = delete;
    SolveDVOStreams &operator=(const SolveDVOStreams &) = delete;

    void setCameraMatrix(float fx, float fy, float cx, float cy) { chk(dvo_tracker_set_intrinsics(tr_, fx, fy, cx, cy)); }
    /* stream s's own calibration (each camera node's setCameraMatrix, SolveDVO.cpp:88-126), before its first frame or after resetStream:
     * the numbers, or the stream's calibration XML */
    void setStreamCameraMatrix(int s, float fx, float fy, float cx, float cy) { chk(dvo_tracker_set_stream_intrinsics(tr_, s, fx, fy, cx, cy)); }
    void setStreamCameraMatrix(int s, const char *calibFile) {
        double k[9];
        readCameraMatrix(calibFile, k);
        setStreamCameraMatrix(s, (float)k[0], (float)k[4], (float)k[2], (float)k[5]);
    }
    /* stream s's cv::undistort (the publisher's K and D, camTopic2PublisherPyD.cpp:88-107) for frames of rows x cols -- the tracker's
     * frame size, anything else is refused; K4 = D5 = NULL: this stream's frames are taken as already undistorted */
    void setStreamUndistort(int s, int rows, int cols, const double *K4, const double *D5) {
        need(rows == tp_.rows && cols == tp_.cols, "setStreamUndistort: calibration for another frame size than the tracker's");
        chk(dvo_tracker_set_stream_undistort(tr_, s, K4, D5));
    }
    /* back to the handle-wide calibration */
    void clearStreamCamera(int s) { chk(dvo_tracker_clear_stream_camera(tr_, s)); }
    /* stream s's ignore mask (dvo_tracker_set_stream_mask; s = -1: every stream): rows x cols bytes of the tracker's frame size, non-zero =
     * "not the world" (the robot's own body, an overlay); NULL removes it.  margin: dilation in level pixels, 2 covers Canny's support.
     * At any time; from the stream's next frame on.  Only the edge maps change: grey, depth and the place descriptors do not */
    void setStreamMask(int s, const unsigned char *mask, int margin = 2) { chk(dvo_tracker_set_stream_mask(tr_, s, mask, margin)); }
    /* how the stream's depth camera sits beside its colour camera, for processFramesRawDepth (dvo_tracker_set_stream_depth_rig: only
     * before the stream's first frame or after resetStream; NULL removes it).  Kc4 / Dc5 of the rig go with setStreamUndistort */
    void setStreamDepthRig(int s, const dvo_depth_rig *rig) { chk(dvo_tracker_set_stream_depth_rig(tr_, s, rig)); }
    /* the 6x6 information matrix with every pose of the calls that follow (dvo_tracker_set_information; off by default) */
    void enableInformation(bool on = true) { chk(dvo_tracker_set_information(tr_, on ? 1 : 0)); }
    /* the record of stream s for the pose its last call returned: H = sum w J J^T, g = J^T W eps, sum eps^2, visible points and the
     * level they were taken on (a first frame: all zero, level -1); covariance: poseCovariance(info.H, info.sum_eps2, info.n_visible, C) */
    struct Information { double H[36]; double g[6]; double sum_eps2; int n_visible; int level; };
    Information lastInformation(int s) {
        Information r{};
        chk(dvo_tracker_get_information(tr_, s, r.H, r.g, &r.sum_eps2, &r.n_visible, &r.level));
        return r;
    }
    /* the views SolveDVO::loop shows, for the calls that follow (dvo_tracker_set_views; off by default) */
    void enableViews(bool on = true) { chk(dvo_tracker_set_views(tr_, on ? 1 : 0)); }
    /* stream s's residue histogram at the pose its last call returned: hist[(int)eps_i + 1] over its reference points (a first frame: all
     * zero, level -1) */
    struct ResidueHistogram { unsigned hist[DVO_VIEW_HISTOGRAM_BINS]; int n_points; int level; };
    ResidueHistogram lastResidueHistogram(int s) {
        ResidueHistogram r{};
        chk(dvo_tracker_get_residue_histogram(tr_, s, r.hist, &r.n_points, &r.level));
        return r;
    }
    /* stream s's view `which` (DVO_VIEW_REPROJ_ON_DT / DVO_VIEW_RESIDUE_HEAT): BGR8, row-major rows x cols x 3 */
    struct View { int rows = 0, cols = 0, level = 0; std::vector<unsigned char> bgr; };
    View lastView(int s, int which) {
        View v;
        chk(dvo_tracker_view_size(tr_, &v.rows, &v.cols, &v.level));
        v.bgr.resize((size_t)v.rows * (size_t)v.cols * 3);
        chk(dvo_tracker_get_view(tr_, s, which, v.bgr.data()));
        return v;
    }
    /* ---- key-frame archive and loop-closure alignment (dvo_tracker_set_archive ...; off by default) ----
     * keep the key frames of the calls that follow in a ring of `capacity` slots in HBM (0: off); matchKeyFrames takes up to maxMatches
     * candidates; pointsCapacity: DVO_MAX_LEVELS entries or NULL (rows_l * cols_l / 8 per slot and level) */
    void enableArchive(int capacity, int maxMatches = 1, const int *pointsCapacity = nullptr) {
        chk(dvo_tracker_set_archive(tr_, capacity, maxMatches, pointsCapacity));
    }
    /* id of stream s's current key frame in the archive; -1: not archived */
    long long keyFrameId(int s) { long long id = -1; chk(dvo_tracker_key_frame_id(tr_, s, &id)); return id; }
    struct ArchivedKeyFrame { int stream = -1; long long frame = 0; std::vector<int> n_points; };
    ArchivedKeyFrame archivedKeyFrame(long long id) {
        ArchivedKeyFrame k;
        k.n_points.assign((size_t)tp_.n_levels, 0);
        chk(dvo_tracker_archive_info(tr_, id, &k.stream, &k.frame, k.n_points.data()));
        return k;
    }
    /* the archived reference list of `level` as 3 x N floats (the contract of dvo_get_ref_level) */
    std::vector<float> archivedPoints(long long id, int level) {
        int n = 0;
        chk(dvo_tracker_archive_get_points(tr_, id, level, nullptr, 0, &n));
        std::vector<float> xyz((size_t)3 * (size_t)n);
        if (n > 0) chk(dvo_tracker_archive_get_points(tr_, id, level, xyz.data(), n, &n));
        return xyz;
    }
    /* one loop-closure candidate: archived key frame keyId against the CURRENT frame of `stream`; R (column-major) and t are the pose to
     * score at (scoreKeyFrames) or the guess in and the aligned pose out (matchKeyFrames), in the convention of the tracker's relative
     * poses; rec is filled by both */
    struct Candidate {
        int stream = 0;
        long long keyId = -1;
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        double t[3] = {0, 0, 0};
        dvo_tracker_score_record rec{};
    };
    /* H, g, sum eps^2 and the visible count of every candidate at its pose on the points of `level`: one launch, one synchronisation */
    void scoreKeyFrames(std::vector<Candidate> &c, int level) {
        packCandidates(c);
        chk(dvo_tracker_score(tr_, (int)c.size(), cs_.data(), ck_.data(), level, cR_.data(), ct_.data(), crec_.data()));
        for (size_t i = 0; i < c.size(); i++) c[i].rec = crec_[i];
    }
    /* the tracker's level schedule for every candidate from its guess, in one alignment launch; tracking is not disturbed */
    void matchKeyFrames(std::vector<Candidate> &c) {
        packCandidates(c);
        std::vector<double> R(cR_.size()), t(ct_.size());
        chk(dvo_tracker_match(tr_, (int)c.size(), cs_.data(), ck_.data(), cR_.data(), ct_.data(), R.data(), t.data(), crec_.data()));
        for (size_t i = 0; i < c.size(); i++) {
            std::copy(R.begin() + 9 * i, R.begin() + 9 * i + 9, c[i].R);
            std::copy(t.begin() + 3 * i, t.begin() + 3 * i + 3, c[i].t);
            c[i].rec = crec_[i];
        }
    }
    /* depth verification: the points of `level` of every candidate's key frame, warped by the candidate's pose, against the DEPTH of the
     * stream's current frame (dvo_tracker_verify; vp = NULL: the default tolerances): one launch, one synchronisation, nothing but the
     * records is written.  Judge a record with dvo_amd::depthVerdict */
    std::vector<dvo_tracker_verify_record> verifyKeyFrames(const std::vector<Candidate> &c, int level,
                                                           const dvo_tracker_verify_params *vp = nullptr) {
        packCandidates(c);
        std::vector<dvo_tracker_verify_record> rec(c.size());
        chk(dvo_tracker_verify(tr_, (int)c.size(), cs_.data(), ck_.data(), level, cR_.data(), ct_.data(), vp, rec.data()));
        return rec;
    }
    /* ---- place descriptors and top-k retrieval (dvo_tracker_set_places ...; needs the archive, off by default) ----
     * one brightness-normalised tiny image of pyramid level `level` per key frame archived from now on; -1: off */
    void enablePlaces(int level) { chk(dvo_tracker_set_places(tr_, level)); }
    /* the D = rows * cols descriptor bytes of an archived key frame, in the frame store's column-major order */
    std::vector<unsigned char> archivedDescriptor(long long id) {
        int D = 0;
        chk(dvo_tracker_archive_get_descriptor(tr_, id, nullptr, 0, &D));
        std::vector<unsigned char> d((size_t)D);
        if (D > 0) chk(dvo_tracker_archive_get_descriptor(tr_, id, d.data(), D, &D));
        return d;
    }
    /* per listed stream the up to k archived key frames nearest to its CURRENT frame, by (distance, key_id): two launches, one
     * synchronisation; the entries feed Candidate{stream, key_id} of matchKeyFrames */
    std::vector<std::vector<dvo_tracker_place>> queryPlaces(const std::vector<int> &streams, int k, long long minFrameGap = 0) {
        const size_t n = streams.size();
        std::vector<dvo_tracker_place> flat(n * (size_t)(k > 0 ? k : 0) + 1);
        std::vector<int> found(n + 1, 0);
        chk(dvo_tracker_query_places(tr_, (int)n, streams.data(), k, minFrameGap, flat.data(), found.data()));
        std::vector<std::vector<dvo_tracker_place>> out(n);
        for (size_t i = 0; i < n; i++) out[i].assign(flat.begin() + i * k, flat.begin() + i * k + found[i]);
        return out;
    }
    /* ---- shift search on place descriptors (dvo_tracker_place_shifts, dvo_tracker_place_guess; needs places) ----
     * per candidate (streams[i], keyIds[i]) the integer shift, |dy|, |dx| <= radius, that best lays the key frame's descriptor onto the
     * stream's current frame, with the SADs to rank or reject on: one launch, one synchronisation, nothing but the records is written */
    std::vector<dvo_tracker_place_shift> placeShifts(const std::vector<int> &streams, const std::vector<long long> &keyIds, int radius) {
        need(streams.size() == keyIds.size(), "placeShifts: one key frame per listed stream");
        std::vector<dvo_tracker_place_shift> rec(streams.size());
        chk(dvo_tracker_place_shifts(tr_, (int)streams.size(), streams.data(), keyIds.data(), radius, rec.data()));
        return rec;
    }
    /* a shift of the descriptor level as the guess of a candidate for matchKeyFrames: the smallest rotation that explains it, t = 0.
     * A first-order guess, not an estimate; host arithmetic only */
    void placeGuess(int stream, int dy, int dx, double *R0, double *t0) { chk(dvo_tracker_place_guess(tr_, stream, dy, dx, R0, t0)); }
    void placeGuess(Candidate &c, const dvo_tracker_place_shift &shift) { placeGuess(c.stream, shift.dy, shift.dx, c.R, c.t); }
    /* "save map / load map" (dvo_tracker_archive_export / _import): the archived key frames `ids` in that order -- or, without a list, every
     * live one in ascending id -- as one self-describing blob, and the key frames of a blob into the next slots of the ring (their new
     * ids, -1 for one the slots cannot hold).  An imported key frame serves score, match, verify, the query and the shift search like the
     * original; nothing changes unless the whole blob is valid */
    std::vector<unsigned char> exportArchive(const std::vector<long long> &ids) { return exportArchive_((int)ids.size(), ids.empty() ? &noId_ : ids.data()); }
    std::vector<unsigned char> exportArchive() { return exportArchive_(0, nullptr); }
    std::vector<long long> importArchive(const std::vector<unsigned char> &blob) {
        struct dvo_archive_blob_info info;
        if (dvo_archive_blob_info(blob.data(), blob.size(), &info) != DVO_OK) throw std::runtime_error(dvo_last_error(nullptr));
        std::vector<long long> ids((size_t)info.n_key_frames, -1);
        int n = 0;
        chk(dvo_tracker_archive_import(tr_, blob.data(), blob.size(), ids.data(), (int)ids.size(), &n));
        return ids;
    }
    void saveArchive(const std::string &path) {
        const std::vector<unsigned char> blob = exportArchive();
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        f.write(reinterpret_cast<const char *>(blob.data()), (std::streamsize)blob.size());
        f.close();
        if (!f) throw std::runtime_error("saveArchive: cannot write " + path);
    }
    std::vector<long long> loadArchive(const std::string &path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("loadArchive: cannot open " + path);
        const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        return importArchive(std::vector<unsigned char>(bytes.begin(), bytes.end()));
    }
    struct KeyFrameOrigin { long long id = -1; int stream = -1; long long frame = 0; };
    KeyFrameOrigin archiveOrigin(long long id) {
        KeyFrameOrigin o;
        chk(dvo_tracker_archive_origin(tr_, id, &o.id, &o.stream, &o.frame));
        return o;
    }
    /* the stream starts over (a new SolveDVO): its next frame is a first frame, its pose chain begins again */
    void resetStream(int s) { chk(dvo_tracker_reset_stream(tr_, s)); gop.at(s) = GOP<double>(); nFrame_.at(s) = 0; }

    /* one received pyramid (RGBDFramePyd: mono8 + mono16, as loadFromFile reads it) per listed stream; returns the latest global pose
     * of each (a first frame: its key-frame pose) */
    std::vector<Pose> processFrames(const std::vector<int> &streams, const std::vector<const RGBDFramePyd *> &frames) {
        need(streams.size() == frames.size(), "processFrames: one frame per listed stream");
        const size_t n = streams.size(), nl = (size_t)tp_.n_levels;
        grey_.resize(n * nl); depth_.resize(n * nl);
        for (size_t i = 0; i < n; i++) {
            need(frames[i] && frames[i]->levels.size() >= nl, "processFrames: frame with too few levels");
            for (size_t l = 0; l < nl; l++) {
                const RGBDFramePyd::Level &L = frames[i]->levels[l];
                grey_[i * nl + l] = dvo_image{L.mono.data(), L.rows, L.cols, DVO_PIX_U8, DVO_LAYOUT_ROW_MAJOR};
                depth_[i * nl + l] = dvo_image{L.depth.data(), L.rows, L.cols, DVO_PIX_U16, DVO_LAYOUT_ROW_MAJOR};
            }
        }
        prepare(n);
        chk(dvo_tracker_step_pyramids(tr_, (int)n, streams.data(), grey_.data(), depth_.data(), 0, R_.data(), t_.data(), lastEvents.data()));
        return compose(streams);
    }
    /* camera frames (BGR8 + depth in metres, as dvo_frames_upload_cameras takes them; flags DVO_UPLOAD_*) */
    std::vector<Pose> processCameraFrames(const std::vector<int> &streams, const std::vector<const unsigned char *> &bgr8,
                                          const std::vector<const float *> &depth_m, int flags = 0) {
        need(streams.size() == bgr8.size() && streams.size() == depth_m.size(), "processCameraFrames: one frame per listed stream");
        prepare(streams.size());
        chk(dvo_tracker_step(tr_, (int)streams.size(), streams.data(), bgr8.data(), depth_m.data(), tp_.rows, tp_.cols, flags, R_.data(),
                             t_.data(), lastEvents.data()));
        return compose(streams);
    }
    /* camera frames as a bgr8 + mono16 topic pair delivers them: 16-bit depth in millimetres goes up as it is
     * (dvo_tracker_step_fmt, DVO_DEPTH_U16: what the pyramid publisher makes of it; with DVO_UPLOAD_DEPTH_RAW holes stay 0) */
    std::vector<Pose> processCameraFrames(const std::vector<int> &streams, const std::vector<const unsigned char *> &bgr8,
                                          const std::vector<const unsigned short *> &depth_mm, int flags = 0) {
        need(streams.size() == bgr8.size() && streams.size() == depth_mm.size(), "processCameraFrames: one frame per listed stream");
        prepare(streams.size());
        chk(dvo_tracker_step_fmt(tr_, (int)streams.size(), streams.data(), reinterpret_cast<const void *const *>(bgr8.data()), DVO_CAM_BGR8,
                                 reinterpret_cast<const void *const *>(depth_mm.data()), DVO_DEPTH_U16, tp_.rows, tp_.cols, flags, R_.data(),
                                 t_.data(), lastEvents.data()));
        return compose(streams);
    }
    /* camera frames whose depth is UNREGISTERED: depth_mm[i] is the raw 16-bit image of the stream's depth camera, in the geometry of its
     * rig (setStreamDepthRig); it is registered to the colour camera on the device (dvo_tracker_step_raw_depth).  flags: 0 or
     * DVO_UPLOAD_DEVICE */
    std::vector<Pose> processFramesRawDepth(const std::vector<int> &streams, const std::vector<const unsigned char *> &bgr8,
                                            const std::vector<const unsigned short *> &depth_mm, int flags = 0) {
        need(streams.size() == bgr8.size() && streams.size() == depth_mm.size(), "processFramesRawDepth: one frame per listed stream");
        prepare(streams.size());
        chk(dvo_tracker_step_raw_depth(tr_, (int)streams.size(), streams.data(), reinterpret_cast<const void *const *>(bgr8.data()), DVO_CAM_BGR8,
                                       reinterpret_cast<const void *const *>(depth_mm.data()), DVO_DEPTH_U16, tp_.rows, tp_.cols, flags,
                                       R_.data(), t_.data(), lastEvents.data()));
        return compose(streams);
    }
    /* ... and with the raw depth in float metres */
    std::vector<Pose> processFramesRawDepth(const std::vector<int> &streams, const std::vector<const unsigned char *> &bgr8,
                                            const std::vector<const float *> &depth_m, int flags = 0) {
        need(streams.size() == bgr8.size() && streams.size() == depth_m.size(), "processFramesRawDepth: one frame per listed stream");
        prepare(streams.size());
        chk(dvo_tracker_step_raw_depth(tr_, (int)streams.size(), streams.data(), reinterpret_cast<const void *const *>(bgr8.data()), DVO_CAM_BGR8,
                                       reinterpret_cast<const void *const *>(depth_m.data()), DVO_DEPTH_F32, tp_.rows, tp_.cols, flags,
                                       R_.data(), t_.data(), lastEvents.data()));
        return compose(streams);
    }
    /* key-frame relative estimate of listed stream i of the last call (cR_64 / cT_64 of its SolveDVO) */
    const double *lastR(size_t i) const { return R_.data() + 9 * i; }
    const double *lastT(size_t i) const { return t_.data() + 3 * i; }
    dvo_tracker *handle() { return tr_; }
    dvo_ctx *context() { return dvo_tracker_context(tr_); }

private:
    void prepare(size_t n) { R_.assign(9 * n, 0.0); t_.assign(3 * n, 0.0); lastEvents.assign(n, 0); }
    /* SolveDVO::processFirstFrame / processFrame's GOP calls (:2014, :2207, :2232, :2239) with the tracker's poses and events */
    std::vector<Pose> compose(const std::vector<int> &streams) {
        std::vector<Pose> out(streams.size());
        for (size_t i = 0; i < streams.size(); i++) {
            const int s = streams[i];
            GOP<double> &g = gop.at(s);
            const int ev = lastEvents[i];
            if (ev == 1) {
                g = GOP<double>();
                nFrame_[s] = 0;
                g.pushAsKeyFrame((int)nFrame_[s], 1, lastR(i), lastT(i));
            } else {
                if (ev >= 2) g.updateMostRecentToKeyFrame(ev);
                g.pushAsOrdinaryFrame((int)nFrame_[s], lastR(i), lastT(i));
            }
            nFrame_[s]++;
            out[i] = g.getGlobalPoseAt(g.size() - 1);
        }
        return out;
    }
    void chk(int rc) { if (rc != DVO_OK) throw std::runtime_error(dvo_tracker_last_error(tr_)); }
    std::vector<unsigned char> exportArchive_(int n, const long long *ids) {
        size_t bytes = 0;
        chk(dvo_tracker_archive_export_size(tr_, n, ids, &bytes));
        std::vector<unsigned char> blob(bytes);
        chk(dvo_tracker_archive_export(tr_, n, ids, blob.data(), blob.size(), &bytes));
        return blob;
    }
    const long long noId_ = -1;                            /* a non-NULL list of no ids: the empty blob, not "every key frame" */
    void packCandidates(const std::vector<Candidate> &c) {
        const size_t n = c.size();
        cs_.resize(n); ck_.resize(n); cR_.resize(9 * n); ct_.resize(3 * n); crec_.resize(n);
        for (size_t i = 0; i < n; i++) {
            cs_[i] = c[i].stream; ck_[i] = c[i].keyId;
            std::copy(c[i].R, c[i].R + 9, cR_.begin() + 9 * i);
            std::copy(c[i].t, c[i].t + 3, ct_.begin() + 3 * i);
        }
    }
    std::vector<int> cs_;
    std::vector<long long> ck_;
    std::vector<double> cR_, ct_;
    std::vector<dvo_tracker_score_record> crec_;
    static void need(bool ok, const char *what) { if (!ok) throw std::runtime_error(what); }
    dvo_tracker *tr_ = nullptr;
    dvo_tracker_params tp_{};
    std::vector<long> nFrame_;
    std::vector<dvo_image> grey_, depth_;
    std::vector<double> R_, t_;
};

/* The legacy photometric Gauss-Newton node (rgbdSubsc): include/RGBDOdometry.h:41-43, src/RGBDOdometry.cpp.  Same method names
 * and per-frame sequence as the reference's eventLoop (:128-211), on the engine's dvo_photo_* entry points; the transport
 * (ROS topics in, odom / path / pose out) stays with the caller, who feeds frames and receives the pose eventLoop publishes.
 * The reference's arithmetic -- defects included -- is the default; RGBDOdometry(true) selects the corrected estimator
 * (the decision per defect: include/dvo_amd.h at dvo_photo_params). */
class RGBDOdometry {
public:
    typedef double TransformRep[16];                 /* Eigen::Transform<double,3,Affine>::matrix(), row-major (RGBDOdometry.h:33) */

    explicit RGBDOdometry(bool fixedDefects = false) : fixed_(fixedDefects) {
        if (dvo_create(nullptr, &ctx_) != DVO_OK) throw std::runtime_error(std::string("dvo_create: ") + dvo_last_error(nullptr));
        identity(T_); identity(base_);
    }
    ~RGBDOdometry() { dvo_destroy(ctx_); }
    RGBDOdometry(const RGBDOdometry &) = delete;
    RGBDOdometry &operator=(const RGBDOdometry &) = delete;

    /* setCameraMatrix (:42-68) keeps fx, fy, cx, cy of params.xml's cameraMatrix */
    void setCameraMatrix(double fx, double fy, double cx, double cy) {
        dvo_photo_params p;
        dvo_photo_params_default(&p);
        p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.fixed = fixed_ ? 1 : 0;
        chk(dvo_photo_configure(ctx_, &p));
        cameraIntrinsicsReady = true;
    }
    /* imageArrivedCallBack: the received colour frame (bgr8, rows x cols x 3 row-major) and depth frame (sensor units) */
    void setRcvdFrame(const unsigned char *bgr8, const unsigned short *depth, int rows, int cols) {
        rcvd_bgr_.assign(bgr8, bgr8 + (size_t)rows * cols * 3);
        rcvd_depth_.assign(depth, depth + (size_t)rows * cols);                  /* taken as is (DVO_DEPTH_U16, DVO_UPLOAD_DEPTH_RAW) */
        rows_ = rows; cols_ = cols;
        isFrameAvailable = true;
    }
    void setRefFrame() { upload(0); isRefFrameAvailable = isPyramidalRefFrameAvailable = true; isJacobiansAvailable = false; }   /* :296-327 */
    void setNowFrame() { upload(1); isNowFrameAvailable = isPyramidalNowFrameAvailable = true; }                                /* :329-357 */
    void computeJacobianAllLevels() {                                            /* :363-398: levels 1..3 */
        need(isPyramidalRefFrameAvailable && cameraIntrinsicsReady, "computeJacobianAllLevels: reference frame / intrinsics missing");
        chk(dvo_photo_set_ref(ctx_, 0, 1, nSelected));
        isJacobiansAvailable = true;
    }
    void gaussNewtonIterations(int level, TransformRep &T) {                     /* :514-597 */
        need(isPyramidalRefFrameAvailable && isPyramidalNowFrameAvailable && isJacobiansAvailable, "gaussNewtonIterations: frames / Jacobians missing");
        need(level != 0, "Critical error, jacobians at level-0 (base) are not computed for complexity reasons");   /* :518 */
        chk(dvo_photo_align(ctx_, 1, &level, 1, T, lastEpsNorms, &lastUpdates));
    }
    /* the body of eventLoop's while (:138-207) for one received frame; returns what it publishes: position = 1000 * translation
     * of base*T (:185-187), orientation = the quaternion of its rotation (:182, :188-191) */
    Pose processFrame() {
        need(isFrameAvailable, "processFrame: no frame received");
        if ((nFrame % refEvery) == 0) {                                          /* :146 ("renew ref-frame every 30 frames": % 10000) */
            mul(base_, T_, base_);                                               /* base = base * T */
            setRefFrame();
            identity(T_);
            computeJacobianAllLevels();
        }
        setNowFrame();
        gaussNewtonIterations(3, T_);                                            /* :162 */
        gaussNewtonIterations(2, T_);                                            /* :163 */
        double S[16];
        mul(base_, T_, S);                                                       /* toSend = base * T :178 */
        double Rc[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rc[i + 3 * j] = S[i * 4 + j];
        Pose p;
        quaternionFromMatrix<double>(Rc, p.qx, p.qy, p.qz, p.qw);
        p.px = 1000 * S[3]; p.py = 1000 * S[7]; p.pz = 1000 * S[11];
        nFrame++;
        isFrameAvailable = false;
        return p;
    }
    /* eventLoop (:128-211) without ROS: pull frames from `next` until it returns false, hand every pose to `publish` */
    template <typename NextFrame, typename Publish>
    void eventLoop(NextFrame next, Publish publish) {
        std::vector<unsigned char> bgr; std::vector<unsigned short> depth; int rows = 0, cols = 0;
        while (next(bgr, depth, rows, cols)) {
            setRcvdFrame(bgr.data(), depth.data(), rows, cols);
            publish(processFrame());
        }
    }
    const double *T() const { return T_; }
    long nFrame = 0;
    int refEvery = 10000;                            /* :146 */
    int nSelected[DVO_MAX_LEVELS] = {0};             /* rows of J per level */
    double lastEpsNorms[64] = {0};
    int lastUpdates = 0;
    dvo_ctx *handle() { return ctx_; }

private:
    void chk(int rc) { if (rc != DVO_OK) throw std::runtime_error(dvo_last_error(ctx_)); }
    static void need(bool ok, const char *what) { if (!ok) throw std::runtime_error(what); }
    static void identity(double *T) { for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.0 : 0.0; }
    static void mul(const double *A, const double *B, double *C) {
        double t[16];
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { double s = 0; for (int k = 0; k < 4; k++) s += A[i * 4 + k] * B[k * 4 + j]; t[i * 4 + j] = s; }
        for (int k = 0; k < 16; k++) C[k] = t[k];
    }
    void upload(int slot) {                          /* 4 levels, INTER_NEAREST at 1, 1/2, 1/4, 1/8 (:313-324, :346-355) */
        need(isFrameAvailable, "Frame not retrived");
        const void *b = rcvd_bgr_.data(), *dp = rcvd_depth_.data();      /* the mono16 frame goes up as 16 bits: the kernels widen it */
        chk(dvo_frames_upload_cameras_fmt(ctx_, slot, 1, &b, DVO_CAM_BGR8, &dp, DVO_DEPTH_U16, rows_, cols_, 4, 0, -1, DVO_UPLOAD_DEPTH_RAW));
    }
    dvo_ctx *ctx_ = nullptr;
    bool fixed_ = false;
    double T_[16], base_[16];
    std::vector<unsigned char> rcvd_bgr_;
    std::vector<unsigned short> rcvd_depth_;
    int rows_ = 0, cols_ = 0;
    bool cameraIntrinsicsReady = false, isFrameAvailable = false, isRefFrameAvailable = false, isNowFrameAvailable = false;
    bool isPyramidalRefFrameAvailable = false, isPyramidalNowFrameAvailable = false, isJacobiansAvailable = false;
};

/* Many photometric nodes in one process (dvo_photo_streams_*, include/dvo_amd.h): K independent copies of RGBDOdometry::processFrame,
 * advanced together.  Per stream the engine keeps the reference, T and nFrame; this class keeps `base` and composes the published
 * pose with the same mul and quaternionFromMatrix as RGBDOdometry, so each stream publishes, bit for bit, what an RGBDOdometry fed
 * that stream's frames alone publishes.  A frame whose new reference is refused (event -1, where RGBDOdometry throws) changes
 * nothing; the stream's previous pose is returned for it. */
class RGBDOdometryStreams {
public:
    std::vector<int> lastEvents;                    /* of the last processFrames call, per listed stream: 1 reference, 0 ordinary, -1 refused */

    explicit RGBDOdometryStreams(int maxStreams, bool fixedDefects = false, int rows = 480, int cols = 640)
        : maxStreams_(maxStreams), fixed_(fixedDefects), rows_(rows), cols_(cols), T_((size_t)maxStreams * 16), base_((size_t)maxStreams * 16) {
        for (int s = 0; s < maxStreams; s++) { identity(&T_[16 * (size_t)s]); identity(&base_[16 * (size_t)s]); }
    }
    ~RGBDOdometryStreams() { if (h_) dvo_photo_streams_destroy(h_); }
    RGBDOdometryStreams(const RGBDOdometryStreams &) = delete;
    RGBDOdometryStreams &operator=(const RGBDOdometryStreams &) = delete;

    /* setCameraMatrix (:42-68); creates the engine's handle, so it comes before the first frame */
    void setCameraMatrix(double fx, double fy, double cx, double cy) {
        dvo_photo_streams_params p;
        dvo_photo_streams_params_default(&p);
        p.photo.fx = fx; p.photo.fy = fy; p.photo.cx = cx; p.photo.cy = cy; p.photo.fixed = fixed_ ? 1 : 0;
        p.ref_every = refEvery;
        p.rows = rows_; p.cols = cols_;
        if (h_) { dvo_photo_streams_destroy(h_); h_ = nullptr; }
        if (dvo_photo_streams_create(&p, maxStreams_, &h_) != DVO_OK)
            throw std::runtime_error(std::string("dvo_photo_streams_create: ") + dvo_photo_streams_last_error(nullptr));
        for (int s = 0; s < maxStreams_; s++) { identity(&T_[16 * (size_t)s]); identity(&base_[16 * (size_t)s]); }
    }
    /* stream s's own camera matrix (each node's setCameraMatrix, :42-68), after setCameraMatrix and before the stream's first frame
     * (or after resetStream) */
    void setStreamCameraMatrix(int s, double fx, double fy, double cx, double cy) {
        need(h_ != nullptr, "setStreamCameraMatrix: camera matrix not set");
        chk(dvo_photo_streams_set_stream_intrinsics(h_, s, fx, fy, cx, cy));
    }
    /* the stream starts over (a new RGBDOdometry) */
    void resetStream(int s) {
        need(h_ != nullptr, "resetStream: camera matrix not set");
        chk(dvo_photo_streams_reset_stream(h_, s));
        identity(&T_.at(16 * (size_t)s)); identity(&base_.at(16 * (size_t)s));
    }
    /* one received frame per listed stream (bgr8 rows x cols x 3 and depth in sensor units, row-major, as setRcvdFrame takes them);
     * returns what each stream's processFrame publishes */
    std::vector<Pose> processFrames(const std::vector<int> &streams, const std::vector<const unsigned char *> &bgr8,
                                    const std::vector<const unsigned short *> &depth) {
        need(h_ != nullptr, "processFrames: camera matrix not set");
        need(streams.size() == bgr8.size() && streams.size() == depth.size(), "processFrames: one frame per listed stream");
        const size_t n = streams.size();
        for (size_t i = 0; i < n; i++) need(depth[i] != nullptr, "processFrames: NULL depth frame");
        Tout_.assign(16 * n, 0.0);
        lastEvents.assign(n, 0);
        /* the mono16 frames go up as 16 bits, as they are (DVO_DEPTH_U16; the engine forces DVO_UPLOAD_DEPTH_RAW) */
        chk(dvo_photo_streams_step_fmt(h_, (int)n, streams.data(), reinterpret_cast<const void *const *>(bgr8.data()), DVO_CAM_BGR8,
                                       reinterpret_cast<const void *const *>(depth.data()), DVO_DEPTH_U16, rows_, cols_, 0, Tout_.data(),
                                       nullptr, nullptr, lastEvents.data()));
        std::vector<Pose> out(n);
        for (size_t i = 0; i < n; i++) {
            double *T = &T_.at(16 * (size_t)streams[i]), *base = &base_.at(16 * (size_t)streams[i]);
            if (lastEvents[i] == 1) mul(base, T, base);                                     /* base = base * T (:146-150) */
            if (lastEvents[i] >= 0) std::copy(Tout_.begin() + 16 * i, Tout_.begin() + 16 * (i + 1), T);
            out[i] = publish(base, T);
        }
        return out;
    }
    const double *T(int s) const { return &T_.at(16 * (size_t)s); }
    int refEvery = 10000;                            /* :146; set before setCameraMatrix */
    dvo_photo_streams *handle() { return h_; }
    dvo_ctx *context() { return dvo_photo_streams_context(h_); }

private:
    /* toSend = base * T (:178), position = 1000 * translation (:185-187), orientation = its rotation's quaternion (:182, :188-191) */
    static Pose publish(const double *base, const double *T) {
        double S[16];
        mul(base, T, S);
        double Rc[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rc[i + 3 * j] = S[i * 4 + j];
        Pose p;
        quaternionFromMatrix<double>(Rc, p.qx, p.qy, p.qz, p.qw);
        p.px = 1000 * S[3]; p.py = 1000 * S[7]; p.pz = 1000 * S[11];
        return p;
    }
    void chk(int rc) { if (rc != DVO_OK) throw std::runtime_error(dvo_photo_streams_last_error(h_)); }
    static void need(bool ok, const char *what) { if (!ok) throw std::runtime_error(what); }
    static void identity(double *T) { for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.0 : 0.0; }
    static void mul(const double *A, const double *B, double *C) {                          /* RGBDOdometry::mul */
        double t[16];
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { double s = 0; for (int k = 0; k < 4; k++) s += A[i * 4 + k] * B[k * 4 + j]; t[i * 4 + j] = s; }
        for (int k = 0; k < 16; k++) C[k] = t[k];
    }
    int maxStreams_;
    bool fixed_;
    int rows_, cols_;
    dvo_photo_streams *h_ = nullptr;
    std::vector<double> T_, base_, Tout_;
};

/* ---- pose graphs (dvo_amd.h, "pose graphs"): the back end for the poses, information records and closures of SolveDVOStreams ----
 * PoseGraph is one graph under construction on the host; PoseGraphs is the dvo_graph_batch handle that solves many of them in one
 * launch and gives the marginal covariances of their poses; edgeChi2 gates a closure candidate with them.  Node poses are world poses {R column-major, t}; an edge (i, j) carries Z ~ T_i^-1 T_j, which is what the tracker returns for
 * key frame i and current frame j. */
struct PoseGraph {
    std::vector<double> poses;                      /* 12 per node */
    std::vector<unsigned char> fixed;
    std::vector<dvo_graph_edge> edges;
    int nodes() const { return (int)fixed.size(); }
    /* a node at the world pose (R column-major, t); returns its index */
    int addNode(const double *R9, const double *t3, bool isFixed = false) {
        poses.insert(poses.end(), R9, R9 + 9);
        poses.insert(poses.end(), t3, t3 + 3);
        fixed.push_back(isFixed ? 1 : 0);
        return nodes() - 1;
    }
    /* a node at T_key Z: the world pose of a frame the tracker placed at Z relative to node `key` */
    int addNodeAfter(int key, const double *R9, const double *t3) {
        const double *K = &poses.at(12 * (size_t)key);
        double R[9], t[3];
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) R[a + 3 * b] = K[a] * R9[3 * b] + K[a + 3] * R9[1 + 3 * b] + K[a + 6] * R9[2 + 3 * b];
            t[a] = K[a] * t3[0] + K[a + 3] * t3[1] + K[a + 6] * t3[2] + K[9 + a];
        }
        return addNode(R, t);
    }
    void addEdge(int i, int j, const double *R9, const double *t3, const double *info36, bool robust) {
        dvo_graph_edge e{};
        e.i = i; e.j = j;
        std::copy(R9, R9 + 9, e.R);
        std::copy(t3, t3 + 3, e.t);
        std::copy(info36, info36 + 36, e.info);
        e.flags = robust ? DVO_GRAPH_EDGE_ROBUST : 0;
        edges.push_back(e);
    }
};
/* an odometry edge key frame i -> frame j from what SolveDVOStreams returned for the frame: its relative pose (R column-major, t) and
 * lastInformation(stream).  false, nothing added: the record gives no information matrix (dvo_graph_information's conditions) */
inline bool addOdometryEdge(PoseGraph &g, int i, int j, const double *R9, const double *t3, const double *H36, double sumEps2, int nVisible) {
    double info[36];
    if (dvo_graph_information(H36, sumEps2, nVisible, info) != DVO_OK) return false;
    g.addEdge(i, j, R9, t3, info, false);
    return true;
}
/* a loop-closure edge archived key frame i -> current frame j from a matched (and verified) candidate of SolveDVOStreams::matchKeyFrames:
 * its aligned pose and score record; robust by default, since a wrong closure is the outlier that Huber is for */
template <class Candidate>
inline bool addClosureEdge(PoseGraph &g, int i, int j, const Candidate &c, bool robust = true) {
    double info[36];
    if (dvo_graph_information(c.rec.H36, c.rec.sum_eps2, c.rec.n_visible, info) != DVO_OK) return false;
    g.addEdge(i, j, c.R, c.t, info, robust);
    return true;
}

/* the gate for a closure candidate (dvo_graph_edge_chi2): chi2 of `edge` between the poses of its two nodes (12 doubles each) under
 * their joint covariance cov144 (PoseGraphs::marginals on {edge.i, edge.j}; nullptr: zero).  false: refused (a number that is not
 * finite, an information matrix or an S without a Cholesky factor) */
inline bool edgeChi2(const double *poseI12, const double *poseJ12, const double *cov144, const dvo_graph_edge &edge, double &chi2,
                     double *r6 = nullptr, double *S36 = nullptr) {
    return dvo_graph_edge_chi2(poseI12, poseJ12, cov144, &edge, r6, S36, &chi2) == DVO_OK;
}

class PoseGraphs {
public:
    PoseGraphs(int maxGraphs, int maxNodesTotal, int maxEdgesTotal) {
        if (dvo_graph_create(maxGraphs, maxNodesTotal, maxEdgesTotal, &h_) != DVO_OK) throw std::runtime_error(dvo_graph_last_error(nullptr));
        dvo_graph_params_default(&params);
    }
    ~PoseGraphs() { if (h_) dvo_graph_destroy(h_); }
    PoseGraphs(const PoseGraphs &) = delete;
    PoseGraphs &operator=(const PoseGraphs &) = delete;
    dvo_graph_params params;                        /* of the solves that follow */
    /* stage graph `graph` on the host (validated there; no device work) */
    void set(int graph, const PoseGraph &g) {
        chk(dvo_graph_set(h_, graph, g.nodes(), g.poses.data(), g.fixed.data(), (int)g.edges.size(), g.edges.data()));
        if ((size_t)graph >= n_.size()) n_.resize((size_t)graph + 1, 0);
        n_[(size_t)graph] = g.nodes();
    }
    /* one upload, DVO_GRAPH_LAUNCHES launch, one copy back, one synchronisation for all listed graphs */
    void solve(const std::vector<int> &graphs) { chk(dvo_graph_solve(h_, &params, (int)graphs.size(), graphs.data())); }
    /* the joint covariance of m nodes of every listed graph at its current poses (dvo_graph_marginals; params' huber_delta, cg_tol and
     * cg_max_iterations): nodes holds m per graph; returns graphs.size() * (6 m)^2 doubles, row-major per graph */
    std::vector<double> marginals(const std::vector<int> &graphs, const std::vector<int> &nodes,
                                  std::vector<dvo_graph_marginal_report> *reports = nullptr) {
        need(!graphs.empty() && !nodes.empty() && nodes.size() % graphs.size() == 0, "marginals: the same number of nodes for every listed graph");
        const size_t m = nodes.size() / graphs.size();
        std::vector<double> cov(graphs.size() * 36 * m * m);
        std::vector<dvo_graph_marginal_report> rep(graphs.size());
        chk(dvo_graph_marginals(h_, &params, (int)graphs.size(), graphs.data(), (int)m, nodes.data(), cov.data(), rep.data()));
        if (reports) *reports = rep;
        return cov;
    }
    std::vector<double> poses(int graph) {
        need(graph >= 0 && (size_t)graph < n_.size() && n_[(size_t)graph] > 0, "poses: the graph was never set");
        std::vector<double> p(12 * (size_t)n_[(size_t)graph]);
        chk(dvo_graph_get_poses(h_, graph, p.data()));
        return p;
    }
    dvo_graph_report report(int graph, std::vector<double> *costTrace = nullptr) {
        dvo_graph_report r{};
        chk(dvo_graph_get_report(h_, graph, &r, nullptr, 0));
        if (costTrace) {
            costTrace->assign((size_t)r.iterations + 1, 0.0);
            chk(dvo_graph_get_report(h_, graph, &r, costTrace->data(), (int)costTrace->size()));
        }
        return r;
    }
private:
    void chk(int rc) { if (rc != DVO_OK) throw std::runtime_error(dvo_graph_last_error(h_)); }
    static void need(bool ok, const char *what) { if (!ok) throw std::runtime_error(what); }
    dvo_graph_batch *h_ = nullptr;
    std::vector<int> n_;
};

/* ---- depth fusion (dvo_amd.h, "depth fusion"): depth frames at the poses of SolveDVOStreams or of a solved PoseGraphs -> a map ----
 * TsdfFrames is a frame list under construction on the host (the images are borrowed, not copied); tsdfIntegrateHost and tsdfExtractHost
 * are the definition on the host; TsdfVolumes is the dvo_tsdf_batch handle that fuses a whole list in one launch.  A pose is a world
 * pose {R column-major, t}: PoseGraphs::poses(graph) + 12 * node goes in as it is. */
struct TsdfFrames {
    std::vector<int> volumes;
    std::vector<const void *> depth;               /* rows x cols each, of one format; borrowed until the call that takes the list returns */
    std::vector<const void *> image;               /* empty, or one colour image per frame for the colour calls: rows x cols of one DVO_CAM_* format */
    std::vector<double> K4, poses12;
    int count() const { return (int)depth.size(); }
    void add(int volume, const void *image, const double *k4, const double *pose12) {
        volumes.push_back(volume);
        depth.push_back(image);
        K4.insert(K4.end(), k4, k4 + 4);
        poses12.insert(poses12.end(), pose12, pose12 + 12);
    }
    /* a frame with its colour image (every frame of a list that goes into a colour call is added this way) */
    void add(int volume, const void *depthImage, const void *colourImage, const double *k4, const double *pose12) {
        add(volume, depthImage, k4, pose12);
        image.push_back(colourImage);
    }
};
inline size_t tsdfVoxels(const dvo_tsdf_volume &v) { return (size_t)v.nx * (size_t)v.ny * (size_t)v.nz; }
/* the frames of the list, in list order, into the words of ONE volume on the host (the list's volume indices play no part).  false:
 * refused (dvo_tsdf_integrate_host's conditions, or words of another size), nothing written */
inline bool tsdfIntegrateHost(const dvo_tsdf_volume &vol, std::vector<unsigned> &words, const TsdfFrames &f, int depthFormat, int rows, int cols,
                              const dvo_tsdf_params *params = nullptr) {
    dvo_tsdf_params p;
    if (params) p = *params; else dvo_tsdf_params_default(&p);
    if (words.size() != tsdfVoxels(vol)) return false;
    return dvo_tsdf_integrate_host(&vol, words.data(), &p, f.count(), f.depth.data(), depthFormat, rows, cols, f.K4.data(), f.poses12.data()) == DVO_OK;
}
/* the surface points of a volume on the host, 3 floats each, in the definition's order.  false: refused */
inline bool tsdfExtractHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &words, int minWeight, std::vector<float> &xyz) {
    long long n = 0;
    if (words.size() != tsdfVoxels(vol) || dvo_tsdf_extract_host(&vol, words.data(), minWeight, nullptr, 0, &n) != DVO_OK) return false;
    xyz.assign(3 * (size_t)n, 0.0f);
    return dvo_tsdf_extract_host(&vol, words.data(), minWeight, xyz.data(), n, &n) == DVO_OK;
}

/* ---- from the map back to depth (dvo_amd.h): fused volumes ray-cast into depth and normal maps ----
 * RaycastViews is a view list under construction; RaycastImages holds what a ray cast returns on the host: the depth images of all
 * views back to back in the call's format (DVO_DEPTH_U16 millimetres or DVO_DEPTH_F32 metres, 0 = a hole) and, when asked for, three
 * floats of world normal per pixel. */
struct RaycastViews {
    std::vector<int> volumes;
    std::vector<double> K4, poses12;
    int count() const { return (int)volumes.size(); }
    void add(int volume, const double *k4, const double *pose12) {
        volumes.push_back(volume);
        K4.insert(K4.end(), k4, k4 + 4);
        poses12.insert(poses12.end(), pose12, pose12 + 12);
    }
};
struct RaycastImages {
    int format = DVO_DEPTH_U16, rows = 0, cols = 0, count = 0;
    std::vector<unsigned char> depth;               /* count images of rows x cols pixels of 2 or 4 bytes */
    std::vector<float> normals;                     /* count x rows x cols x 3, or empty */
    int imageFormat = DVO_CAM_BGR8;
    std::vector<unsigned char> image;               /* of a colour call: count images of rows x cols pixels of 3 bytes or, DVO_CAM_MONO8, 1; else empty */
    size_t colourBytes() const { return (size_t)rows * (size_t)cols * (imageFormat == DVO_CAM_MONO8 ? 1 : 3); }
    const unsigned char *imageOf(int view) const { return image.empty() ? nullptr : image.data() + colourBytes() * (size_t)view; }
    /* room for the colour images of a call after shape(), and their pointer list */
    void shapeColour(int format, std::vector<void *> &ip) {
        imageFormat = format;
        image.assign(depth.empty() ? 0 : colourBytes() * (size_t)count, 0);
        ip.clear();
        for (int i = 0; !image.empty() && i < count; i++) ip.push_back(image.data() + colourBytes() * (size_t)i);
    }
    size_t imageBytes() const { return (size_t)rows * (size_t)cols * (format == DVO_DEPTH_U16 ? 2 : 4); }
    const void *depthOf(int view) const { return depth.data() + imageBytes() * (size_t)view; }
    const float *normalsOf(int view) const { return normals.empty() ? nullptr : normals.data() + 3 * (size_t)rows * (size_t)cols * (size_t)view; }
    /* room for the images of a call, and the pointer lists a C call takes */
    void shape(int depthFormat, int r, int c, int n, bool withNormals, std::vector<void *> &dp, std::vector<float *> &np) {
        format = depthFormat; rows = r; cols = c; count = n;
        const bool ok = r > 0 && c > 0 && n > 0;
        depth.assign(ok ? imageBytes() * (size_t)n : 0, 0);
        normals.assign(ok && withNormals ? 3 * (size_t)r * (size_t)c * (size_t)n : 0, 0.0f);
        dp.clear(); np.clear();
        for (int i = 0; ok && i < n; i++) {
            dp.push_back(depth.data() + imageBytes() * (size_t)i);
            if (withNormals) np.push_back(normals.data() + 3 * (size_t)r * (size_t)c * (size_t)i);
        }
    }
};
/* the views of the list of ONE volume on the host (the list's volume indices play no part): the definition.  false: refused
 * (dvo_raycast_host's conditions, or words of another size) */
inline bool tsdfRaycastHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &words, const RaycastViews &v, int depthFormat, int rows, int cols,
                            bool withNormals, RaycastImages &out, const dvo_raycast_params *params = nullptr) {
    dvo_raycast_params p;
    if (params) p = *params; else dvo_raycast_params_default(&p);
    if (words.size() != tsdfVoxels(vol) || (depthFormat != DVO_DEPTH_U16 && depthFormat != DVO_DEPTH_F32)) return false;
    std::vector<void *> dp;
    std::vector<float *> np;
    out.shape(depthFormat, rows, cols, v.count(), withNormals, dp, np);
    if (dp.empty()) return false;
    return dvo_raycast_host(&vol, words.data(), &p, v.count(), depthFormat, rows, cols, v.K4.data(), v.poses12.data(), dp.data(),
                            withNormals ? np.data() : nullptr) == DVO_OK;
}

/* ---- the surface as a triangle mesh (dvo_amd.h): vertices, 3 floats each, and triangles, 3 vertex numbers each, in the definition's
 * order; a triangle's normal (right-hand rule) points to the viewer's side ---- */
struct Mesh {
    std::vector<float> xyz;
    std::vector<int> tri;
    std::vector<unsigned char> rgb;                 /* of a colour call: R, G, B per vertex; else empty */
    size_t vertices() const { return xyz.size() / 3; }
    size_t triangles() const { return tri.size() / 3; }
};
/* the mesh of a volume on the host: the definition; one call for the counts and one for the mesh.  false: refused (dvo_mesh_host's
 * conditions, or words of another size) */
inline bool tsdfMeshHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &words, int minWeight, Mesh &out) {
    long long nv = 0, nt = 0;
    if (words.size() != tsdfVoxels(vol) || dvo_mesh_host(&vol, words.data(), minWeight, nullptr, 0, nullptr, 0, &nv, &nt) != DVO_OK) return false;
    out.xyz.assign(3 * (size_t)nv, 0.0f);
    out.tri.assign(3 * (size_t)nt, 0);
    return dvo_mesh_host(&vol, words.data(), minWeight, nv ? out.xyz.data() : nullptr, nv, nt ? out.tri.data() : nullptr, nt, &nv, &nt) == DVO_OK;
}

/* ---- colour in the map (dvo_amd.h): the three definitions on the host with colour words (64 bits per voxel) beside the words ---- */
inline bool tsdfIntegrateColourHost(const dvo_tsdf_volume &vol, std::vector<unsigned> &words, std::vector<unsigned long long> &colours,
                                    const TsdfFrames &f, int depthFormat, int imageFormat, int rows, int cols, const dvo_tsdf_params *params = nullptr) {
    dvo_tsdf_params p;
    if (params) p = *params; else dvo_tsdf_params_default(&p);
    if (words.size() != tsdfVoxels(vol) || colours.size() != words.size() || f.image.size() != f.depth.size()) return false;
    return dvo_colour_integrate_host(&vol, words.data(), colours.data(), &p, f.count(), f.depth.data(), depthFormat, f.image.data(), imageFormat, rows,
                                     cols, f.K4.data(), f.poses12.data()) == DVO_OK;
}
inline bool tsdfRaycastColourHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &words, const std::vector<unsigned long long> &colours,
                                  const RaycastViews &v, int depthFormat, int imageFormat, int rows, int cols, bool withNormals, RaycastImages &out,
                                  const dvo_raycast_params *params = nullptr) {
    dvo_raycast_params p;
    if (params) p = *params; else dvo_raycast_params_default(&p);
    if (words.size() != tsdfVoxels(vol) || colours.size() != words.size() || (depthFormat != DVO_DEPTH_U16 && depthFormat != DVO_DEPTH_F32)) return false;
    std::vector<void *> dp, ip;
    std::vector<float *> np;
    out.shape(depthFormat, rows, cols, v.count(), withNormals, dp, np);
    out.shapeColour(imageFormat, ip);
    if (dp.empty()) return false;
    return dvo_colour_raycast_host(&vol, words.data(), colours.data(), &p, v.count(), depthFormat, rows, cols, v.K4.data(), v.poses12.data(), dp.data(),
                                   withNormals ? np.data() : nullptr, ip.data(), imageFormat) == DVO_OK;
}
inline bool tsdfMeshColourHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &words, const std::vector<unsigned long long> &colours,
                               int minWeight, Mesh &out) {
    long long nv = 0, nt = 0;
    if (words.size() != tsdfVoxels(vol) || colours.size() != words.size() ||
        dvo_colour_mesh_host(&vol, words.data(), colours.data(), minWeight, nullptr, nullptr, 0, nullptr, 0, &nv, &nt) != DVO_OK)
        return false;
    out.xyz.assign(3 * (size_t)nv, 0.0f);
    out.rgb.assign(3 * (size_t)nv, 0);
    out.tri.assign(3 * (size_t)nt, 0);
    return dvo_colour_mesh_host(&vol, words.data(), colours.data(), minWeight, nv ? out.xyz.data() : nullptr, nv ? out.rgb.data() : nullptr, nv,
                                nt ? out.tri.data() : nullptr, nt, &nv, &nt) == DVO_OK;
}

/* ---- distance fields (dvo_amd.h): the three definitions on the host.  false: refused (the C functions' conditions, or words of
 * another size) ---- */
inline bool esdfHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &voxels, std::vector<unsigned> &words, const dvo_esdf_params *params = nullptr) {
    dvo_esdf_params p;
    if (params) p = *params; else dvo_esdf_params_default(&p);
    if (voxels.size() != tsdfVoxels(vol)) return false;
    std::vector<unsigned> out(voxels.size());
    if (dvo_esdf_host(&vol, voxels.data(), &p, out.data()) != DVO_OK) return false;
    words.swap(out);
    return true;
}
inline bool esdfDistancesHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &words, std::vector<float> &metres) {
    if (words.size() != tsdfVoxels(vol)) return false;
    std::vector<float> out(words.size());
    if (dvo_esdf_distances_host(&vol, words.data(), out.data()) != DVO_OK) return false;
    metres.swap(out);
    return true;
}
inline bool esdfQueryHost(const dvo_tsdf_volume &vol, const std::vector<unsigned> &words, const std::vector<double> &points,
                          std::vector<dvo_esdf_sample> &records) {
    if (words.size() != tsdfVoxels(vol) || points.empty() || points.size() % 3 != 0) return false;
    std::vector<dvo_esdf_sample> out(points.size() / 3);
    if (dvo_esdf_query_host(&vol, words.data(), (int)out.size(), points.data(), out.data()) != DVO_OK) return false;
    records.swap(out);
    return true;
}

class TsdfVolumes {
public:
    TsdfVolumes(int maxVolumes, long long maxVoxelsTotal) {
        if (dvo_tsdf_create(maxVolumes, maxVoxelsTotal, &h_) != DVO_OK) throw std::runtime_error(dvo_tsdf_last_error(nullptr));
        dvo_tsdf_params_default(&params);
    }
    ~TsdfVolumes() { if (h_) dvo_tsdf_destroy(h_); }
    TsdfVolumes(const TsdfVolumes &) = delete;
    TsdfVolumes &operator=(const TsdfVolumes &) = delete;
    dvo_tsdf_params params;                         /* of the integrations that follow */
    /* the volume's geometry; it is cleared.  Volumes sit in the pool back to back in the order they are set */
    void setVolume(int volume, const dvo_tsdf_volume &v) {
        chk(dvo_tsdf_set_volume(h_, volume, &v));
        if ((size_t)volume >= n_.size()) n_.resize((size_t)volume + 1, 0);
        n_[(size_t)volume] = tsdfVoxels(v);
        if ((size_t)volume >= dims_.size()) dims_.resize((size_t)volume + 1, 1);
        dims_[(size_t)volume] = v.nz;
    }
    void clear(int volume) { chk(dvo_tsdf_clear(h_, volume)); }
    /* one upload, DVO_TSDF_INTEGRATE_LAUNCHES launch, one synchronisation for the whole list; flags: 0 (host images) or DVO_UPLOAD_DEVICE */
    void integrate(const TsdfFrames &f, int depthFormat, int rows, int cols, int flags = 0) {
        chk(dvo_tsdf_integrate(h_, &params, f.count(), f.volumes.data(), f.depth.data(), depthFormat, rows, cols, f.K4.data(), f.poses12.data(), flags));
    }
    /* the volume's surface points, 3 floats each, in the definition's order: one extraction for the count and one for the points */
    std::vector<float> points(int volume, int minWeight = 1) {
        long long n = 0;
        chk(dvo_tsdf_extract_points(h_, volume, minWeight, nullptr, 0, &n));
        std::vector<float> xyz(3 * (size_t)n);
        if (n > 0) chk(dvo_tsdf_extract_points(h_, volume, minWeight, xyz.data(), n, &n));
        return xyz;
    }
    std::vector<unsigned> voxels(int volume) {
        need(volume >= 0 && (size_t)volume < n_.size() && n_[(size_t)volume] > 0, "voxels: the volume was never set");
        std::vector<unsigned> w(n_[(size_t)volume]);
        chk(dvo_tsdf_get_voxels(h_, volume, w.data()));
        return w;
    }
    void setVoxels(int volume, const std::vector<unsigned> &w) {
        need(volume >= 0 && (size_t)volume < n_.size() && n_[(size_t)volume] == w.size() && !w.empty(), "setVoxels: nx * ny * nz words of a set volume");
        chk(dvo_tsdf_set_voxels(h_, volume, w.data()));
    }
    /* view i of the list looks at volume views.volumes[i]: one upload, DVO_RAYCAST_LAUNCHES launch, one copy back and one
     * synchronisation for the whole list (device-resident outputs: dvo_raycast_views with DVO_UPLOAD_DEVICE) */
    RaycastImages raycast(const RaycastViews &v, int depthFormat, int rows, int cols, bool withNormals = false, const dvo_raycast_params *p = nullptr) {
        dvo_raycast_params prm;
        if (p) prm = *p; else dvo_raycast_params_default(&prm);
        need(depthFormat == DVO_DEPTH_U16 || depthFormat == DVO_DEPTH_F32, "raycast: an unknown depth format");
        RaycastImages out;
        std::vector<void *> dp;
        std::vector<float *> np;
        out.shape(depthFormat, rows, cols, v.count(), withNormals, dp, np);
        chk(dvo_raycast_views(h_, &prm, v.count(), v.volumes.data(), depthFormat, rows, cols, v.K4.data(), v.poses12.data(), dp.empty() ? nullptr : dp.data(),
                              withNormals ? np.data() : nullptr, 0));
        return out;
    }
    /* the volume's triangle mesh on the device: one extraction with zero capacities for the counts and one for the mesh, each of
     * DVO_MESH_LAUNCHES launches and one synchronisation (device-resident outputs: dvo_mesh_extract with DVO_UPLOAD_DEVICE) */
    Mesh mesh(int volume, int minWeight = 1) {
        long long nv = 0, nt = 0;
        chk(dvo_mesh_extract(h_, volume, minWeight, nullptr, 0, nullptr, 0, &nv, &nt, 0));
        Mesh out;
        out.xyz.assign(3 * (size_t)nv, 0.0f);
        out.tri.assign(3 * (size_t)nt, 0);
        chk(dvo_mesh_extract(h_, volume, minWeight, nv ? out.xyz.data() : nullptr, nv, nt ? out.tri.data() : nullptr, nt, &nv, &nt, 0));
        return out;
    }
    /* the handle gets its colour pool (8 bytes per voxel); from then on setVolume and clear also zero the colour words */
    void enableColour() { chk(dvo_colour_enable(h_)); }
    /* integrate() with the list's colour images (TsdfFrames::add with two images), all of imageFormat */
    void integrateColour(const TsdfFrames &f, int depthFormat, int imageFormat, int rows, int cols, int flags = 0) {
        need(f.image.size() == f.depth.size(), "integrateColour: one colour image per frame");
        chk(dvo_colour_integrate(h_, &params, f.count(), f.volumes.data(), f.depth.data(), depthFormat, f.image.data(), imageFormat, rows, cols,
                                 f.K4.data(), f.poses12.data(), flags));
    }
    std::vector<unsigned long long> colours(int volume) {
        need(volume >= 0 && (size_t)volume < n_.size() && n_[(size_t)volume] > 0, "colours: the volume was never set");
        std::vector<unsigned long long> c(n_[(size_t)volume]);
        chk(dvo_colour_get_words(h_, volume, c.data()));
        return c;
    }
    void setColours(int volume, const std::vector<unsigned long long> &c) {
        need(volume >= 0 && (size_t)volume < n_.size() && n_[(size_t)volume] == c.size() && !c.empty(), "setColours: nx * ny * nz words of a set volume");
        chk(dvo_colour_set_words(h_, volume, c.data()));
    }
    /* raycast() with a colour image per view in RaycastImages::image */
    RaycastImages raycastColour(const RaycastViews &v, int depthFormat, int imageFormat, int rows, int cols, bool withNormals = false,
                                const dvo_raycast_params *p = nullptr) {
        dvo_raycast_params prm;
        if (p) prm = *p; else dvo_raycast_params_default(&prm);
        need(depthFormat == DVO_DEPTH_U16 || depthFormat == DVO_DEPTH_F32, "raycastColour: an unknown depth format");
        RaycastImages out;
        std::vector<void *> dp, ip;
        std::vector<float *> np;
        out.shape(depthFormat, rows, cols, v.count(), withNormals, dp, np);
        out.shapeColour(imageFormat, ip);
        chk(dvo_colour_raycast_views(h_, &prm, v.count(), v.volumes.data(), depthFormat, rows, cols, v.K4.data(), v.poses12.data(),
                                     dp.empty() ? nullptr : dp.data(), withNormals ? np.data() : nullptr, ip.empty() ? nullptr : ip.data(), imageFormat, 0));
        return out;
    }
    /* mesh() with R, G, B per vertex in Mesh::rgb */
    Mesh meshColour(int volume, int minWeight = 1) {
        long long nv = 0, nt = 0;
        chk(dvo_colour_mesh_extract(h_, volume, minWeight, nullptr, nullptr, 0, nullptr, 0, &nv, &nt, 0));
        Mesh out;
        out.xyz.assign(3 * (size_t)nv, 0.0f);
        out.rgb.assign(3 * (size_t)nv, 0);
        out.tri.assign(3 * (size_t)nt, 0);
        chk(dvo_colour_mesh_extract(h_, volume, minWeight, nv ? out.xyz.data() : nullptr, nv ? out.rgb.data() : nullptr, nv,
                                    nt ? out.tri.data() : nullptr, nt, &nv, &nt, 0));
        return out;
    }
    /* the handle gets its distance-field pool (4 bytes per voxel); every reader below throws until updateEsdf() has listed the volume,
     * and again after its words changed */
    void enableEsdf() { chk(dvo_esdf_enable(h_)); }
    /* the Euclidean distance fields of the listed volumes from their words as they are now: one upload, DVO_ESDF_UPDATE_LAUNCHES
     * launches and one synchronisation for the whole list */
    void updateEsdf(const std::vector<int> &volumes, const dvo_esdf_params *p = nullptr) {
        dvo_esdf_params prm;
        if (p) prm = *p; else dvo_esdf_params_default(&prm);
        chk(dvo_esdf_update(h_, &prm, (int)volumes.size(), volumes.data()));
    }
    /* the volume's ESDF words: d2 in bits 0..23, DVO_ESDF_INSIDE, DVO_ESDF_UNKNOWN */
    std::vector<unsigned> esdfWords(int volume) {
        need(volume >= 0 && (size_t)volume < n_.size() && n_[(size_t)volume] > 0, "esdfWords: the volume was never set");
        std::vector<unsigned> w(n_[(size_t)volume]);
        chk(dvo_esdf_get_words(h_, volume, w.data()));
        return w;
    }
    /* metres of the nz z-planes from iz0, nz * ny * nx floats in index order, converted on the device: one launch, one synchronisation */
    std::vector<float> esdfDistances(int volume, int iz0, int nz) {
        need(volume >= 0 && (size_t)volume < n_.size() && n_[(size_t)volume] > 0 && nz >= 1, "esdfDistances: a set volume and nz >= 1");
        std::vector<float> d(n_[(size_t)volume] / (size_t)dims_[(size_t)volume] * (size_t)nz);
        chk(dvo_esdf_get_distances(h_, volume, iz0, nz, d.data(), 0));
        return d;
    }
    /* the batched point query (points: 3 doubles each, world coordinates): one launch, one synchronisation */
    std::vector<dvo_esdf_sample> esdfQuery(int volume, const std::vector<double> &points) {
        need(!points.empty() && points.size() % 3 == 0, "esdfQuery: three doubles per point, at least one point");
        std::vector<dvo_esdf_sample> out(points.size() / 3);
        chk(dvo_esdf_query(h_, volume, (int)out.size(), points.data(), out.data(), 0));
        return out;
    }
    /* kernel launches and host synchronisations of the last integrate, points, raycast or mesh call, colour variants included, or of
     * the last updateEsdf, esdfDistances or esdfQuery */
    void stats(int &launches, int &syncs) { chk(dvo_tsdf_stats(h_, &launches, &syncs)); }
private:
    void chk(int rc) { if (rc != DVO_OK) throw std::runtime_error(dvo_tsdf_last_error(h_)); }
    static void need(bool ok, const char *what) { if (!ok) throw std::runtime_error(what); }
    dvo_tsdf_batch *h_ = nullptr;
    std::vector<size_t> n_;
    std::vector<int> dims_;                         /* nz of every set volume */
};

/* ---- frame-to-model alignment (dvo_amd.h): depth frames against ray-cast model views, projective point-to-plane ICP ----
 * IcpViews is a view list under construction (the images are borrowed, not copied: host memory, or device memory for
 * IcpAligner::align with DVO_UPLOAD_DEVICE); IcpResult holds what an alignment returns; icpAlignHost is the definition on the host;
 * IcpAligner is the dvo_icp_batch handle that aligns a whole list with two launches per sweep and one synchronisation.
 * The front end of a sensor's depth frame (dvo_amd.h, "preparing a depth frame"): IcpPrepared holds filtered depth and now-frame
 * normals, icpPrepareHost is the definition, IcpAligner::prepare / prepareDevice the device call; a view list with nowNormals (one per
 * view: setNowNormals) is aligned with the normal gate at normalCosMin. */
struct IcpViews {
    std::vector<const void *> nowDepth, modelDepth; /* rows x cols each, every list of one format */
    std::vector<const float *> modelNormals;        /* 3 floats per pixel, world axes, (0, 0, 0) = none */
    std::vector<double> K4, modelPoses12, startPoses12;
    std::vector<const float *> nowNormals;          /* empty: ungated; else one per view, 3 floats per pixel, the now camera's axes */
    double normalCosMin = 0.0;                      /* of the gate: in [-1, 1] */
    int count() const { return (int)nowDepth.size(); }
    bool gated() const { return !nowNormals.empty(); }
    /* the now normals of view i (every view needs them once one has them) */
    void setNowNormals(int i, const float *normals) {
        if (nowNormals.size() < nowDepth.size()) nowNormals.resize(nowDepth.size(), nullptr);
        nowNormals.at((size_t)i) = normals;
    }
    void add(const void *now, const void *model, const float *normals, const double *k4, const double *modelPose12, const double *startPose12) {
        nowDepth.push_back(now);
        modelDepth.push_back(model);
        modelNormals.push_back(normals);
        K4.insert(K4.end(), k4, k4 + 4);
        modelPoses12.insert(modelPoses12.end(), modelPose12, modelPose12 + 12);
        startPoses12.insert(startPoses12.end(), startPose12, startPose12 + 12);
    }
};
struct IcpResult {
    std::vector<double> poses12;                    /* 12 per view: {R column-major, t}, camera to world */
    std::vector<dvo_icp_record> records;            /* one per view; info in the tangent order (v, w) of a world-frame left increment */
    void shape(int n) {
        poses12.assign(12 * (size_t)(n > 0 ? n : 0), 0.0);
        records.assign((size_t)(n > 0 ? n : 0), dvo_icp_record{});
    }
};
/* the views of the list on the host: the definition.  false: refused (dvo_icp_align_host's conditions) */
inline bool icpAlignHost(const IcpViews &v, int nowFormat, int modelFormat, int rows, int cols, IcpResult &out, const dvo_icp_params *params = nullptr) {
    dvo_icp_params p;
    if (params) p = *params; else dvo_icp_params_default(&p);
    out.shape(v.count());
    if (v.count() < 1 || (v.gated() && v.nowNormals.size() != v.nowDepth.size())) return false;
    return dvo_icp_align_gated_host(&p, v.count(), nowFormat, modelFormat, rows, cols, v.K4.data(), v.nowDepth.data(), v.modelDepth.data(),
                                    v.modelNormals.data(), v.modelPoses12.data(), v.startPoses12.data(), v.gated() ? v.nowNormals.data() : nullptr,
                                    v.normalCosMin, out.poses12.data(), out.records.data()) == DVO_OK;
}
/* what preparing a list of depth images returns on the host: per image rows x cols float metres (0 = a hole) and, when asked for,
 * 3 rows x cols floats of normals in the now camera's axes ((0, 0, 0) = none) */
struct IcpPrepared {
    std::vector<std::vector<float>> depth, normals;
    std::vector<float *> depthPtr, normalsPtr;
    void shape(int n, int rows, int cols, bool withNormals) {
        const size_t c = (size_t)(n > 0 ? n : 0), px = rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols : 0;
        depth.assign(c, std::vector<float>(px, 0.0f));
        normals.assign(withNormals ? c : 0, std::vector<float>(3 * px, 0.0f));
        depthPtr.clear();
        normalsPtr.clear();
        for (auto &d : depth) depthPtr.push_back(d.data());
        for (auto &q : normals) normalsPtr.push_back(q.data());
    }
};
/* the definition on the host (params NULL: the default).  K4: 4 doubles per image.  false: refused (dvo_icp_prepare_host's conditions) */
inline bool icpPrepareHost(const std::vector<const void *> &depth, int depthFormat, int rows, int cols, const std::vector<double> &K4, IcpPrepared &out,
                           bool withNormals = true, const dvo_icp_prepare_params *params = nullptr) {
    dvo_icp_prepare_params p;
    if (params) p = *params; else dvo_icp_prepare_params_default(&p);
    const int n = (int)depth.size();
    out.shape(n, rows, cols, withNormals);
    if (n < 1 || K4.size() != 4 * depth.size() || rows < 1 || cols < 1) return false;
    return dvo_icp_prepare_host(&p, n, depthFormat, rows, cols, K4.data(), depth.data(), out.depthPtr.data(),
                                withNormals ? out.normalsPtr.data() : nullptr) == DVO_OK;
}

class IcpAligner {
public:
    explicit IcpAligner(int maxViews) {
        if (dvo_icp_create(maxViews, &h_) != DVO_OK) throw std::runtime_error(dvo_icp_last_error(nullptr));
        dvo_icp_params_default(&params);
        dvo_icp_prepare_params_default(&prepareParams);
    }
    ~IcpAligner() { if (h_) dvo_icp_destroy(h_); }
    IcpAligner(const IcpAligner &) = delete;
    IcpAligner &operator=(const IcpAligner &) = delete;
    dvo_icp_params params;                          /* of the alignments that follow */
    /* one upload, DVO_ICP_LAUNCHES_PER_SWEEP launches per sweep, one copy back and one synchronisation for the whole list; flags: 0 (host
     * images) or DVO_UPLOAD_DEVICE (device images, read in place: what dvo_raycast_views(..., DVO_UPLOAD_DEVICE) wrote) */
    IcpResult align(const IcpViews &v, int nowFormat, int modelFormat, int rows, int cols, int flags = 0) {
        IcpResult out;
        out.shape(v.count());
        if (v.gated() && v.nowNormals.size() != v.nowDepth.size()) throw std::runtime_error("now normals: one per view");
        chk(dvo_icp_align_gated(h_, &params, v.count(), nowFormat, modelFormat, rows, cols, v.K4.data(), v.nowDepth.data(), v.modelDepth.data(),
                                v.modelNormals.data(), v.modelPoses12.data(), v.startPoses12.data(), v.gated() ? v.nowNormals.data() : nullptr,
                                v.normalCosMin, out.poses12.data(), out.records.data(), flags));
        return out;
    }
    dvo_icp_prepare_params prepareParams;           /* of the prepare calls that follow */
    /* host images: DVO_ICP_PREPARE_LAUNCHES launches (one without normals), one copy back, one synchronisation */
    IcpPrepared prepare(const std::vector<const void *> &depth, int depthFormat, int rows, int cols, const std::vector<double> &K4, bool withNormals = true) {
        IcpPrepared out;
        if (K4.size() != 4 * depth.size()) throw std::runtime_error("K4: four doubles per image");
        out.shape((int)depth.size(), rows, cols, withNormals);
        chk(dvo_icp_prepare(h_, &prepareParams, (int)depth.size(), depthFormat, rows, cols, K4.data(), depth.data(), out.depthPtr.data(),
                            withNormals ? out.normalsPtr.data() : nullptr, 0));
        return out;
    }
    /* device images into device buffers of the caller (normalsOut may be empty: none), read and written in place, nothing copied back */
    void prepareDevice(const std::vector<const void *> &depth, int depthFormat, int rows, int cols, const std::vector<double> &K4,
                       const std::vector<float *> &depthOut, const std::vector<float *> &normalsOut) {
        if (K4.size() != 4 * depth.size() || depthOut.size() != depth.size() || (!normalsOut.empty() && normalsOut.size() != depth.size()))
            throw std::runtime_error("K4, depthOut and normalsOut: one entry per image");
        chk(dvo_icp_prepare(h_, &prepareParams, (int)depth.size(), depthFormat, rows, cols, K4.data(), depth.data(), depthOut.data(),
                            normalsOut.empty() ? nullptr : normalsOut.data(), DVO_UPLOAD_DEVICE));
    }
    /* kernel launches and host synchronisations of the last align or prepare */
    void stats(int &launches, int &syncs) { chk(dvo_icp_stats(h_, &launches, &syncs)); }
private:
    void chk(int rc) { if (rc != DVO_OK) throw std::runtime_error(dvo_icp_last_error(h_)); }
    dvo_icp_batch *h_ = nullptr;
};

}  // namespace dvo_amd
#endif
