// Defining stand-in for the part of {fmt}'s core API that the reference's utils/flog.h uses (fmt 9+:
// format_string, string_view, format). Test infrastructure, our own code: oracle/_ref/ref_blocks*
// puts this directory ahead of tests/stubs on its include path, because the reference's
// RationalResampler logs its plan through flog::debug, so format() and the format string's members
// are instantiated and must have bodies. format() returns the format string itself; the probe's
// flog::logImpl (oracle/ref_standins.cpp) discards the message. tests/stubs/fmt/core.h stays the
// declaration-only header of the overlay syntax checks.
#pragma once
#include <string>
#include <string_view>
#include <type_traits>
namespace fmt {
using string_view = std::string_view;
template <class... Args>
struct basic_format_string {
    template <class S, class = std::enable_if_t<std::is_convertible_v<const S&, std::string_view>>>
    basic_format_string(const S& s) : str(s) {}
    operator string_view() const { return str; }
    std::string_view str;
};
template <class T> struct type_identity { using type = T; };
template <class... Args>
using format_string = basic_format_string<typename type_identity<Args>::type...>;
template <class... Args>
std::string format(format_string<Args...> f, Args&&...) {
    return std::string(string_view(f));
}
}  // namespace fmt
