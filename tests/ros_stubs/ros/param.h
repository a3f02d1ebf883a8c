#pragma once
#include <string>
#include <vector>
namespace ros {
namespace param {
bool get(const std::string &key, double &v);
bool get(const std::string &key, std::vector<double> &v);
}
}
