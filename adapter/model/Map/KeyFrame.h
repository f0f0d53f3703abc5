// Test model only — stands in for Modules/Map/KeyFrame.h with the members the adapter uses
// (getId, getPose/setPose, getKeyPoint(s), getDepthMeasure, get/setEstimatedDepthScale,
// getMapPoints/setMapPoint, getCalibration, getInvSigma2, getNumberOfScales, clone, and the depth
// image: getDepthIm, getDepthScale, getDepthMeasure(x, y, scaled)).
#pragma once

#include <cmath>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "Mapping/Frame.h"

class KeyFrame {
public:
    explicit KeyFrame(Frame &f)
        : vKeys_(f.getKeyPoints()), vDepthMeasurements_(f.getDepthMeasurements()), vMapPoints_(f.getMapPoints()),
          calibration_(f.getCalibration()), phcalibration_(f.getPHCalibration()),
          imageDepthScale_(f.getDepthScale()), estimatedDepthScale_(f.getEstimatedDepthScale()),
          Tcw_(f.getPose()), nId_(nNextId_++), depthIm_(f.getDepthIm()) {
        const int n = f.getNumberOfScales();
        for (int i = 0; i < n; i++) {
            vScaleFactor_.push_back(f.getScaleFactor(i));
            vInvSigma2_.push_back(f.getInvSigma2(i));
        }
    }
    // KeyFrame.cc:68-99: every MapPoint of the slots cloned (distinct from the Map's objects)
    KeyFrame(const KeyFrame &other)
        : vKeys_(other.vKeys_), vDepthMeasurements_(other.vDepthMeasurements_), calibration_(other.calibration_),
          phcalibration_(other.phcalibration_), imageDepthScale_(other.imageDepthScale_),
          estimatedDepthScale_(other.estimatedDepthScale_), Tcw_(other.Tcw_), nId_(other.nId_),
          vScaleFactor_(other.vScaleFactor_), vInvSigma2_(other.vInvSigma2_), depthIm_(other.depthIm_) {   // the data shared (KeyFrame.cc:75)
        for (const auto &pMP : other.vMapPoints_)
            vMapPoints_.emplace_back(pMP ? std::shared_ptr<MapPoint>(pMP->clone()) : nullptr);
    }
    KeyFrame *clone() const { return new KeyFrame(*this); }

    Sophus::SE3f getPose() { return Tcw_; }
    void setPose(Sophus::SE3f &Tcw) { Tcw_ = Tcw; }
    cv::KeyPoint getKeyPoint(size_t idx) { return vKeys_[idx]; }
    std::vector<cv::KeyPoint> &getKeyPoints() { return vKeys_; }
    float getDepthMeasure(size_t idx) { return vDepthMeasurements_[idx]; }
    std::vector<float> &getDepthMeasurements() { return vDepthMeasurements_; }
    // real images (KeyFrame.cc:156-158); setDepthIm / getDepthScale are the model's plumbing
    cv::Mat getDepthIm() { return depthIm_.clone(); }
    void setDepthIm(cv::Mat &im, double imageDepthScale) { depthIm_ = im.clone(); imageDepthScale_ = imageDepthScale; }
    double getDepthScale() { return imageDepthScale_; }
    // KeyFrame.cc:181-202 over Interpolate (Geometry.cc:607-620): the depth image lookup; the
    // simulation sets no image and the call throws.  `scaled` returns the plain depth,
    // !scaled multiplies by imageDepthScale_ (the flag reads backwards in the reference)
    double getDepthMeasure(float x, float y, bool scaled = true) {
        if (depthIm_.empty()) throw std::runtime_error("Depth image is not initialized.");
        if (x >= depthIm_.cols || y >= depthIm_.rows) {
            std::cout << x << " " << y << std::endl;
            throw std::out_of_range("Pixel coordinates are out of range.");
        }
        const float *mat = depthIm_.ptr<float>(0);
        const int cols = depthIm_.cols;
        float x_, y_;
        const float _x = std::modf(x, &x_), _y = std::modf(y, &y_);
        // where the reference would read outside the buffer the model throws instead
        if (!(x >= 0.f) || !(y >= 0.f) || ((long long)y_ + 1) * cols + (long long)x_ + 1 >= (long long)depthIm_.rows * cols)
            throw std::out_of_range("Pixel coordinates read outside the depth image.");
        const float w00 = (1.f - _x) * (1.f - _y);
        const float w01 = (1.f - _x) * _y;
        const float w10 = _x * (1.f - _y);
        const float w11 = 1.f - w00 - w01 - w10;
        const float ground_truth_depth = mat[(int)y_ * cols + (int)x_] * w00 + mat[(int)y_ * cols + (int)x_ + 1] * w10 +
                                         mat[((int)y_ + 1) * cols + (int)x_] * w01 + mat[((int)y_ + 1) * cols + (int)x_ + 1] * w11;
        const double depth = static_cast<double>(ground_truth_depth) / 100;
        return scaled ? depth : depth * imageDepthScale_;
    }
    double getEstimatedDepthScale() { return estimatedDepthScale_; }
    void setEstimatedDepthScale(double scale) { estimatedDepthScale_ = scale; }
    std::vector<std::shared_ptr<MapPoint>> &getMapPoints() { return vMapPoints_; }
    void setMapPoint(size_t idx, std::shared_ptr<MapPoint> pMP) { vMapPoints_[idx] = pMP; }
    std::shared_ptr<MapPoint> getMapPoint(size_t idx) { return vMapPoints_[idx]; }
    std::shared_ptr<CameraModel> getCalibration() { return calibration_; }
    std::shared_ptr<CameraModel> getPHCalibration() { return phcalibration_; }
    long unsigned int getId() { return nId_; }
    float getScaleFactor(int octave) { return vScaleFactor_[octave]; }
    float getInvSigma2(int octave) { return vInvSigma2_[octave]; }
    int getNumberOfScales() { return (int)vScaleFactor_.size(); }
    static void resetIdCounter() { nNextId_ = 0; }   // model only

private:
    std::vector<cv::KeyPoint> vKeys_;
    std::vector<float> vDepthMeasurements_;
    std::vector<std::shared_ptr<MapPoint>> vMapPoints_;
    std::shared_ptr<CameraModel> calibration_, phcalibration_;
    double imageDepthScale_ = 1.0, estimatedDepthScale_ = 1.0;
    Sophus::SE3f Tcw_;
    long unsigned int nId_;
    std::vector<float> vScaleFactor_, vInvSigma2_;
    cv::Mat depthIm_;
    static inline long unsigned int nNextId_ = 0;   // KeyFrame.cc:25
};
