// Stand-in g2o::Sim3 for the Sim3Optimizer drop-in harness: g2o's accessor names (types/sim3.h:280-290) over stand-ins of the two Eigen types they
// return, so that the template overload of Sim3Optimizer::OptimizeSim3 is executed as a build with g2o would execute it.
#pragma once

namespace Eigen {

class Quaterniond {
public:
    double& x() { return c[0]; }
    double& y() { return c[1]; }
    double& z() { return c[2]; }
    double& w() { return c[3]; }
    double x() const { return c[0]; }
    double y() const { return c[1]; }
    double z() const { return c[2]; }
    double w() const { return c[3]; }

private:
    double c[4] = {0, 0, 0, 1};
};

class Vector3d {
public:
    double& operator[](int i) { return v[i]; }
    double operator[](int i) const { return v[i]; }

private:
    double v[3] = {0, 0, 0};
};

}  // namespace Eigen

namespace g2o {

struct Sim3 {
    const Eigen::Vector3d& translation() const { return t; }
    Eigen::Vector3d& translation() { return t; }
    const Eigen::Quaterniond& rotation() const { return r; }
    Eigen::Quaterniond& rotation() { return r; }
    const double& scale() const { return s; }
    double& scale() { return s; }

protected:
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s = 1.0;
};

}  // namespace g2o
