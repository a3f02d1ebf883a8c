// UG_GPU_matcher_ugsm.cpp -- the UG_matcher_gpu node on top of libugsm (catkin build only; not
// compiled in the GPU image, which has no ROS).  Same node / topic / service / parameter names and
// message layouts as /root/reference/src/gpu_matcher/UG_GPU_matcher.cpp (:48-61,:742); the body of
// each callback is: convert to rgb8 (or, for an encoding the library reads as it is, hand the payload over in place with its input
// format) -> one call into the MatchGPULib shim -> wrap the returned
// planes in 32FC1 images.  Written from the reference's interface, not from its source text: one
// persistent matcher object instead of one per callback, cv::Mat headers over the returned planes
// instead of per-pixel at<float>() loops, the service path fills the whole fovea stack (U6).
//
// Not in the reference: the parameter `frames_in_flight` (default 1 = the reference's behaviour, one blocking match() per callback,
// UG_GPU_matcher.cpp:423).  With n > 1 the topic path enqueues every synchronised pair into the library's queue (include/ugsm.h:
// ugsm_enqueue_*_managed through the shim's enqueueMatch / enqueueStack) and publishes results as they complete, in arrival order, a
// frame or n - 1 later; the callback blocks only while n pairs are outstanding, and a 1 ms wall timer publishes what finishes between
// frames.  16 MP full mode, one MI355X: 67-70 pairs/s blocking, ~160 pairs/s with frames in flight (bench.py, pcie_inclusive).
//
// Not in the reference either: the parameter `publish_cloud` (default 0).  With it on, and frames_in_flight > 1, the topic path enqueues the
// cloud forms (ugsm_enqueue_*_cloud_managed through enqueueMatchCloud / enqueueStackCloud) and publishes every frame's coloured cloud --
// doReconstructionRGB's, or the merged cloud of the fovea stack -- on output_pointcloud as a sensor_msgs::PointCloud2 filled from
// ugsm_done_cloud, as INTEGRATION.md section 7 shows.  cloud_P1 / cloud_P2: the two 3x4 projection matrices, row-major, 12 numbers each (required);
// cloud_sampling, cloud_format (0 PCL32, 1 XYZRGB16), cloud_compact, cloud_min_conf, cloud_z_min, cloud_z_max: ugsm_cloud_params;
// cloud_max_points: the cap (0 = the dense size); cloud_only = 1: the planes are neither downloaded nor published.
//
// Nor this: the parameter `lr_check_tau` (default 0 = off).  With tau > 0 the blocking full-mode paths (topic and service) run the LR check for the call:
// both directions in one lockstep call (ugsm_match_full_checked), the confidence plane zeroed where the match does not point back within tau pixels.
// With frames_in_flight > 1 the full-mode topic path enqueues the checked queue forms with that tau (the shim's enqueueMatchChecked, and
// enqueueMatchCheckedCloud with publish_cloud: a compact cloud with cloud_min_conf > 0 then leaves the marked pixels out); tau is read per frame.
//
// Nor this: the parameter `seed_level` (default -1 = off).  With a level s >= 0 the blocking full-mode topic path keeps every frame's result and starts the
// next frame of the same size at level s from it (the shim's matchSeeded: ugsm_match_full_seeded) instead of from the zero seed at the top level; the
// first frame, a frame of another size and a frame after a failed call are matched cold.
#include <cv_bridge/cv_bridge.h>
#include <image_transport/image_transport.h>
#include <image_transport/subscriber_filter.h>
#include <message_filters/sync_policies/approximate_time.h>
#include <message_filters/synchronizer.h>
#include <ros/param.h>
#include <ros/ros.h>
#include <sensor_msgs/PointCloud2.h>
#include <sensor_msgs/image_encodings.h>
#include <stereo_msgs/DisparityImage.h>
#include <ug_stereomatcher/GetDisparitiesGPU.h>
#include <ug_stereomatcher/foveatedstack.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "MatchGPULib_ugsm.hpp"

namespace enc = sensor_msgs::image_encodings;
using ug_stereomatcher::foveatedstack;

class GPU_matcher {
public:
    GPU_matcher(int argc, char **argv)
        : it_(nh_), imL_sub_(it_, "input_left_image", 1), imR_sub_(it_, "input_right_image", 1),
          sync_(Policy(1), imL_sub_, imR_sub_)
    {
        // frames_in_flight: read once, at start-up (it sizes the context); handed to the shim as "-inflight=N"
        nh_.getParam("frames_in_flight", frames_in_flight_);
        if (frames_in_flight_ < 1) frames_in_flight_ = 1;
        inflight_arg_ = "-inflight=" + std::to_string(frames_in_flight_);
        std::vector<char *> av(argv, argv + argc);
        while (av.size() < 3) av.push_back(const_cast<char *>(av.size() == 2 ? "7" : ""));  // (argv[2] stays the number of fovea levels)
        av.push_back(const_cast<char *>(inflight_arg_.c_str()));
        mgpu_.reset(new MatchGPULib((int)av.size(), av.data()));
        if (frames_in_flight_ > 1) poll_timer_ = nh_.createWallTimer(ros::WallDuration(0.001), &GPU_matcher::pollTimer, this);
        for (const char *t : {"output_stackH", "output_stackV", "output_stackC", "output_stackL_pyramid", "output_stackR_pyramid"})
            stack_pub_[t] = nh_.advertise<foveatedstack>(t, 1);
        for (const char *t : {"output_disparityH", "output_disparityV", "output_disparityC"})
            disp_pub_[t] = nh_.advertise<stereo_msgs::DisparityImage>(t, 1);
        nh_.getParam("publish_cloud", publish_cloud_);
        if (publish_cloud_ && frames_in_flight_ > 1) {
            std::vector<double> p1, p2;
            if (!ros::param::get("~cloud_P1", p1) || !ros::param::get("~cloud_P2", p2) || p1.size() != 12 || p2.size() != 12) {
                ROS_ERROR("publish_cloud needs cloud_P1 and cloud_P2 (12 numbers each): no cloud is published");
                publish_cloud_ = 0;
            } else {
                std::memset(&cloud_spec_, 0, sizeof cloud_spec_);
                for (int k = 0; k < 12; k++) { cloud_spec_.P1[k] = p1[k]; cloud_spec_.P2[k] = p2[k]; }
                ugsm_default_cloud_params(&cloud_spec_.params);
                int cloud_only = 0, max_points = 0;
                double v;
                nh_.getParam("cloud_sampling", cloud_spec_.params.sampling);
                nh_.getParam("cloud_format", cloud_spec_.params.format);
                nh_.getParam("cloud_compact", cloud_spec_.params.compact);
                if (ros::param::get("~cloud_min_conf", v)) cloud_spec_.params.min_conf = (float)v;
                if (ros::param::get("~cloud_z_min", v)) cloud_spec_.params.z_min = (float)v;
                if (ros::param::get("~cloud_z_max", v)) cloud_spec_.params.z_max = (float)v;
                nh_.getParam("cloud_max_points", max_points);
                nh_.getParam("cloud_only", cloud_only);
                cloud_spec_.max_points = max_points;
                cloud_spec_.want_planes = cloud_only ? 0 : 1;
                cloud_pub_ = nh_.advertise<sensor_msgs::PointCloud2>("output_pointcloud", 1);
            }
        } else {
            publish_cloud_ = 0;  // (the blocking path has no cloud: getPointCloud's node, or INTEGRATION.md section 7's slot-level calls)
        }
        srv_ = nh_.advertiseService("get_disparities_srv", &GPU_matcher::disparitySrv, this);
        sync_.registerCallback(boost::bind(&GPU_matcher::mainRoutine, this, _1, _2));
    }

private:
    typedef message_filters::sync_policies::ApproximateTime<sensor_msgs::Image, sensor_msgs::Image> Policy;
    ros::NodeHandle nh_;
    image_transport::ImageTransport it_;
    image_transport::SubscriberFilter imL_sub_, imR_sub_;
    message_filters::Synchronizer<Policy> sync_;
    ros::ServiceServer srv_;
    std::map<std::string, ros::Publisher> stack_pub_, disp_pub_;
    std::unique_ptr<MatchGPULib> mgpu_;
    int frames_in_flight_ = 1;
    int publish_cloud_ = 0;
    ugsm_queue_cloud cloud_spec_;
    ros::Publisher cloud_pub_;
    std::string inflight_arg_;
    ros::WallTimer poll_timer_;
    struct InFlight { std_msgs::Header hl, hr; };
    std::map<uint64_t, InFlight> in_flight_;  // headers of the frames whose results have not been published yet
    uint64_t next_tag_ = 0;
    float **last_ = nullptr;  // seed_level >= 0: the last full-mode result of the topic path (last_w_ x last_h_), the next frame's prior
    int last_w_ = 0, last_h_ = 0;

    int foveated()
    {  // re-read on every call, default 0 with a warning (reference :96-102)
        int f = 0;
        if (!nh_.getParam("foveated", f)) ROS_WARN("foveated option has not been set. Matcher is on non-foveated mode!");
        return f;
    }
    float lr_check_tau()
    {  // (not in the reference) re-read on every call like `foveated`; > 0: the blocking full-mode matches check left against right in one
       // lockstep call (the shim's match(L, R, fov, tau): ugsm_match_full_checked) and dispC / output_disparityC carry the checked confidence
        double tau = 0.0;
        ros::param::get("~lr_check_tau", tau);
        return (float)tau;
    }
    int seed_level()
    {  // (not in the reference) re-read on every call like `foveated`; >= 0: the level a frame is started at from the last frame's result
        int s = -1;
        nh_.getParam("seed_level", s);
        return s;
    }
    void drop_last()
    {
        if (last_) { for (int c = 0; c < 3; c++) free(last_[c]); free(last_); }
        last_ = nullptr;
    }
    static sensor_msgs::Image plane_msg(float *p, int rows, int cols, const std_msgs::Header &h)
    {
        cv_bridge::CvImage out(h, enc::TYPE_32FC1, cv::Mat(rows, cols, CV_32FC1, p));
        return *out.toImageMsg();
    }
    // (levels*fovH) x fovW, finest level first
    foveatedstack stack_msg(float ***st, int plane, const std_msgs::Header &h, int imW, int imH, bool dims)
    {
        const int F = mgpu_->getFoveateLevel(), fw = mgpu_->getFoveaWidth(), fh = mgpu_->getFoveaHeight();
        cv::Mat m(F * fh, fw, CV_32FC1);
        for (int k = 0; k < F; k++) std::memcpy(m.ptr<float>(k * fh), st[k][plane], sizeof(float) * fw * fh);
        foveatedstack s;
        s.header = h;
        s.image_stack = *cv_bridge::CvImage(h, enc::TYPE_32FC1, m).toImageMsg();
        if (dims) { s.im_width = imW; s.im_height = imH; s.roi_width = fw; s.roi_height = fh; s.num_levels = F; }
        return s;
    }
    // (levels*fovH) x fovW stack straight from the library's plane (already in the published layout)
    foveatedstack stack_msg(float *plane, int rows_per_level, const std_msgs::Header &h, int imW, int imH)
    {
        const int F = mgpu_->getFoveateLevel(), fw = mgpu_->getFoveaWidth(), fh = mgpu_->getFoveaHeight();
        foveatedstack s;
        s.header = h;
        s.image_stack = plane_msg(plane, F * rows_per_level, fw, h);
        s.im_width = imW; s.im_height = imH; s.roi_width = fw; s.roi_height = fh; s.num_levels = F;
        return s;
    }
    // the frame's cloud as an unorganised PointCloud2: one copy out of the library's page-locked records
    static sensor_msgs::PointCloud2 cloud_msg(const ugsm_cloud_result &c, bool dense, const std_msgs::Header &h)
    {
        sensor_msgs::PointCloud2 msg;
        msg.header = h;
        msg.height = 1;
        msg.width = (uint32_t)c.stored;
        msg.is_bigendian = false;
        msg.is_dense = dense;
        msg.point_step = (uint32_t)c.point_step;
        msg.row_step = msg.point_step * msg.width;
        const char *names[4] = {"x", "y", "z", "rgb"};
        const uint32_t offsets[4] = {0, 4, 8, c.point_step == 32 ? 16u : 12u};
        msg.fields.resize(4);
        for (int k = 0; k < 4; k++) {
            msg.fields[k].name = names[k];
            msg.fields[k].offset = offsets[k];
            msg.fields[k].datatype = sensor_msgs::PointField::FLOAT32;  // rgb: the packed word, read as a float (PCL's convention)
            msg.fields[k].count = 1;
        }
        msg.data.resize((size_t)c.point_step * (size_t)c.stored);
        if (c.stored > 0) std::memcpy(msg.data.data(), c.points, msg.data.size());
        return msg;
    }
    // publishes the oldest finished frame; false if there is none (block == false: or it has not finished)
    bool publishNext(bool block)
    {
        MatchGPULib::Done d;
        if (in_flight_.empty() || !mgpu_->nextDone(block, &d)) return false;
        const InFlight f = in_flight_[d.tag];
        in_flight_.erase(d.tag);
        if (d.status != UGSM_OK) {  // the frame's call failed (reference: exit()): the frame is dropped, the node lives on
            ROS_ERROR("ugsm: frame %llu dropped: %s", (unsigned long long)d.tag, ugsm_status_string(d.status));
            return true;
        }
        if (d.has_cloud) cloud_pub_.publish(cloud_msg(d.cloud, cloud_spec_.params.compact != 0, f.hl));
        if (!d.planes[0]) return true;  // (a cloud pair enqueued without its planes: cloud_only)
        if (d.foveated) {
            const int fh = mgpu_->getFoveaHeight();
            if (d.pyramids) {
                stack_pub_["output_stackL_pyramid"].publish(stack_msg(d.planes[3], 3 * fh, f.hl, d.cols, d.rows));
                stack_pub_["output_stackR_pyramid"].publish(stack_msg(d.planes[4], 3 * fh, f.hr, d.cols, d.rows));
            }
            stack_pub_["output_stackH"].publish(stack_msg(d.planes[0], fh, f.hl, d.cols, d.rows));
            stack_pub_["output_stackV"].publish(stack_msg(d.planes[1], fh, f.hr, d.cols, d.rows));
            stack_pub_["output_stackC"].publish(stack_msg(d.planes[2], fh, f.hl, d.cols, d.rows));
        } else {
            const char *topics[3] = {"output_disparityH", "output_disparityV", "output_disparityC"};
            for (int i = 0; i < 3; i++) {
                stereo_msgs::DisparityImage m;
                m.header = (i == 1) ? f.hr : f.hl;
                m.image = plane_msg(d.planes[i], d.rows, d.cols, m.header);
                disp_pub_[topics[i]].publish(m);
            }
        }
        return true;
    }
    void pollTimer(const ros::WallTimerEvent &) { while (publishNext(false)) {} }
    void drain() { while (!in_flight_.empty() && publishNext(true)) {} }

    static void free_stack(float ***st, int F)
    {
        for (int k = 0; k < F; k++) { for (int i = 0; i < 3; i++) free(st[k][i]); free(st[k]); }
        free(st);
    }

    // The input format of a pair of messages when the library reads their encoding as it is (rgb8, bgr8, rgba8, bgra8, mono8, and the float
    // images 32FC3 / 32FC1, whose samples become level 0 of the pyramid without a rounding to bytes: the payloads go to the library in
    // place, no cv_bridge copy); -1: convert with cv_bridge::toCvCopy(.., RGB8) as the reference does.  A float payload the library would
    // refuse -- a step that is no multiple of 4, data that is not 4-byte aligned -- takes the conversion too.
    static bool float_rows_ok(const sensor_msgs::Image &m) { return m.step % 4 == 0 && reinterpret_cast<uintptr_t>(m.data.data()) % 4 == 0; }
    static int in_place_format(const sensor_msgs::Image &l, const sensor_msgs::Image &r)
    {
        const int fmt = ugsm_input_format_from_encoding(l.encoding.c_str());
        if (fmt < 0 || r.encoding != l.encoding) return -1;
        if ((fmt == UGSM_INPUT_RGB32F || fmt == UGSM_INPUT_MONO32F) && !(float_rows_ok(l) && float_rows_ok(r))) return -1;
        return fmt;
    }

    bool disparitySrv(ug_stereomatcher::GetDisparitiesGPU::Request &req, ug_stereomatcher::GetDisparitiesGPU::Response &rsp)
    {
        const int fmt = in_place_format(req.imL, req.imR);
        if (fmt >= 0) {
            mgpu_->setInputFormat(fmt);
            return serve(MatchGPULib::view(req.imL), MatchGPULib::view(req.imR), rsp);
        }
        cv_bridge::CvImagePtr L, R;
        try { L = cv_bridge::toCvCopy(req.imL, enc::RGB8); R = cv_bridge::toCvCopy(req.imR, enc::RGB8); }
        catch (cv_bridge::Exception &) { ROS_ERROR("Could not convert from '%s' to 'rgb8'.", req.imL.encoding.c_str()); return false; }
        mgpu_->setInputFormat(UGSM_INPUT_RGB8);
        return serve(L, R, rsp);
    }

    template <class Img>
    bool serve(const Img &L, const Img &R, ug_stereomatcher::GetDisparitiesGPU::Response &rsp)
    {
        const int fov = foveated();
        mgpu_->setFoveated(fov);
        drain();  // (pipelined topic path: the slots belong to the queue while frames are in flight; publish them first)
        if (fov == 1) {
            float ***st = mgpu_->matchStack(L, R);
            if (!st) return false;
            rsp.fdispH = stack_msg(st, 0, L->header, 0, 0, false);
            rsp.fdispV = stack_msg(st, 1, R->header, 0, 0, false);
            rsp.fdispC = stack_msg(st, 2, L->header, 0, 0, false);
            free_stack(st, mgpu_->getFoveateLevel());
        } else {
            float **fin = mgpu_->match(L, R, fov, lr_check_tau());  // (tau <= 0: the plain match)
            if (!fin) return false;
            rsp.dispH.image = plane_msg(fin[0], L->image.rows, L->image.cols, L->header); rsp.dispH.header = L->header;
            rsp.dispV.image = plane_msg(fin[1], L->image.rows, L->image.cols, R->header); rsp.dispV.header = R->header;
            rsp.dispC.image = plane_msg(fin[2], L->image.rows, L->image.cols, L->header); rsp.dispC.header = L->header;
            for (int i = 0; i < 3; i++) free(fin[i]);
            free(fin);
        }
        return true;
    }

    void mainRoutine(const sensor_msgs::ImageConstPtr &imL, const sensor_msgs::ImageConstPtr &imR)
    {
        const int fmt = in_place_format(*imL, *imR);
        if (fmt >= 0) {  // (the queue's managed calls copy the payloads before they return: the messages need not outlive the call)
            mgpu_->setInputFormat(fmt);
            route(MatchGPULib::view(*imL), MatchGPULib::view(*imR));
            return;
        }
        cv_bridge::CvImagePtr L, R;
        try { L = cv_bridge::toCvCopy(imL, enc::RGB8); R = cv_bridge::toCvCopy(imR, enc::RGB8); }
        catch (cv_bridge::Exception &) { ROS_ERROR("Could not convert from '%s' to 'rgb8'.", imL->encoding.c_str()); return; }
        mgpu_->setInputFormat(UGSM_INPUT_RGB8);
        route(L, R);
    }

    template <class Img>
    void route(const Img &L, const Img &R)
    {
        const int fov = foveated();
        mgpu_->setFoveated(fov);
        const ros::WallTime t0 = ros::WallTime::now();
        if (frames_in_flight_ > 1) {
            // pipelined: enqueue (the images are copied before the call returns), publish what has finished, block only while
            // frames_in_flight pairs are outstanding
            const uint64_t tag = next_tag_++;
            if (fov == 1) mgpu_->initStack(L, R);
            // (a status other than UGSM_OK = the pair was REJECTED and nothing is outstanding under the tag: include/ugsm.h, ugsm_enqueue_*)
            // (the cloud forms carry no pyramid stacks: with publish_cloud the foveated path publishes the H, V, C stacks and the cloud)
            // (lr_check_tau > 0, full mode: the checked forms, the pair's own tau; the node publishes the left camera's field only)
            const float tau = fov == 1 ? 0.0f : lr_check_tau();
            const int st = tau > 0.0f ? (publish_cloud_ ? mgpu_->enqueueMatchCheckedCloud(L, R, tau, false, cloud_spec_, tag) : mgpu_->enqueueMatchChecked(L, R, tau, false, tag))
                         : publish_cloud_ ? (fov == 1 ? mgpu_->enqueueStackCloud(L, R, cloud_spec_, tag) : mgpu_->enqueueMatchCloud(L, R, cloud_spec_, tag))
                                          : (fov == 1 ? mgpu_->enqueueStack(L, R, true, tag) : mgpu_->enqueueMatch(L, R, tag));
            if (st != UGSM_OK) { ROS_ERROR("ugsm enqueue failed: %s", ugsm_status_string(st)); return; }
            in_flight_[tag] = InFlight{L->header, R->header};
            while (publishNext(false)) {}
            while (mgpu_->outstanding() >= frames_in_flight_ && publishNext(true)) {}
            return;
        }
        if (fov == 1) {
            mgpu_->initStack(L, R);
            const int F = mgpu_->getFoveateLevel(), fw = mgpu_->getFoveaWidth(), fh = mgpu_->getFoveaHeight();
            // caller-allocated [14][3][fovW*fovH] as the reference node does
            float ***lf = (float ***)malloc(14 * sizeof(float **)), ***rf = (float ***)malloc(14 * sizeof(float **));
            for (int k = 0; k < 14; k++) {
                lf[k] = (float **)malloc(3 * sizeof(float *)); rf[k] = (float **)malloc(3 * sizeof(float *));
                for (int c = 0; c < 3; c++) { lf[k][c] = (float *)malloc(sizeof(float) * fw * fh); rf[k][c] = (float *)malloc(sizeof(float) * fw * fh); }
            }
            float ***st = mgpu_->matchStackPyramid(L, R, lf, rf);
            ROS_INFO("Foveated Disparity took %f Seconds", (ros::WallTime::now() - t0).toSec());
            if (st) {
                auto pyr = [&](float ***p, const std_msgs::Header &h) {  // (F*3*fovH) x fovW, rows [level][channel][row]
                    cv::Mat m(F * 3 * fh, fw, CV_32FC1);
                    for (int k = 0; k < F; k++) for (int c = 0; c < 3; c++) std::memcpy(m.ptr<float>((k * 3 + c) * fh), p[k][c], sizeof(float) * fw * fh);
                    foveatedstack s; s.header = h; s.image_stack = *cv_bridge::CvImage(h, enc::TYPE_32FC1, m).toImageMsg();
                    s.im_width = L->image.cols; s.im_height = L->image.rows; s.roi_width = fw; s.roi_height = fh; s.num_levels = F;
                    return s;
                };
                stack_pub_["output_stackL_pyramid"].publish(pyr(lf, L->header));
                stack_pub_["output_stackR_pyramid"].publish(pyr(rf, R->header));
                stack_pub_["output_stackH"].publish(stack_msg(st, 0, L->header, L->image.cols, L->image.rows, true));
                stack_pub_["output_stackV"].publish(stack_msg(st, 1, R->header, L->image.cols, L->image.rows, true));
                stack_pub_["output_stackC"].publish(stack_msg(st, 2, L->header, L->image.cols, L->image.rows, true));
                free_stack(st, F);
            }
            for (int k = 0; k < 14; k++) { for (int c = 0; c < 3; c++) { free(lf[k][c]); free(rf[k][c]); } free(lf[k]); free(rf[k]); }
            free(lf); free(rf);
        } else {
            const int sl = seed_level();
            const bool seeded = sl >= 0 && last_ && last_w_ == L->image.cols && last_h_ == L->image.rows;
            float **fin = seeded ? mgpu_->matchSeeded(L, R, last_, sl)
                                 : mgpu_->match(L, R, fov, lr_check_tau());  // (tau <= 0: the plain match)
            ROS_INFO("Non Foveated Disparity took %f Seconds", (ros::WallTime::now() - t0).toSec());
            drop_last();  // (a failed call too: the next frame is matched cold)
            if (!fin) return;
            const char *topics[3] = {"output_disparityH", "output_disparityV", "output_disparityC"};
            for (int i = 0; i < 3; i++) {
                stereo_msgs::DisparityImage d;
                d.header = (i == 1) ? R->header : L->header;
                d.image = plane_msg(fin[i], L->image.rows, L->image.cols, d.header);
                disp_pub_[topics[i]].publish(d);
            }
            if (sl >= 0) {  // the next frame's prior
                last_ = fin;
                last_w_ = L->image.cols;
                last_h_ = L->image.rows;
                return;
            }
            for (int i = 0; i < 3; i++) free(fin[i]);
            free(fin);
        }
    }
};

int main(int argc, char **argv)
{
    ros::init(argc, argv, "RH_GPU_matcher");
    GPU_matcher matcher(argc, argv);
    while (ros::ok()) ros::spin();
    return 0;
}
