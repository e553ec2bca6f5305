// flan/vec2.h -- a pair of numbers with component-wise arithmetic: the position type of Audio::stereo_spatialize (the reference's
// flan/Utility/vec2.h for the parts that method uses).  vec2 holds floats, vec2d doubles.
#pragma once
#include <cmath>
#include <complex>

namespace flan {

template<typename T>
struct vec2Base
	{
	T _x, _y;

	vec2Base() : _x( 0 ), _y( 0 ) {}
	vec2Base( T x, T y ) : _x( x ), _y( y ) {}
	template<typename O> vec2Base( const vec2Base<O> & o ) : _x( T( o.x() ) ), _y( T( o.y() ) ) {}      // vec2 -> vec2d and back
	vec2Base( std::complex<T> c ) : _x( c.real() ), _y( c.imag() ) {}
	operator std::complex<T>() const { return std::complex<T>( _x, _y ); }

	T & x() { return _x; }
	T & y() { return _y; }
	const T & x() const { return _x; }
	const T & y() const { return _y; }

	vec2Base operator+( const vec2Base & r ) const { return vec2Base( _x + r._x, _y + r._y ); }
	vec2Base operator-( const vec2Base & r ) const { return vec2Base( _x - r._x, _y - r._y ); }
	vec2Base operator-() const { return vec2Base( -_x, -_y ); }
	vec2Base operator*( const T s ) const { return vec2Base( _x * s, _y * s ); }
	vec2Base operator/( const T s ) const { return vec2Base( _x / s, _y / s ); }

	T mag() const { return std::sqrt( _x * _x + _y * _y ); }
	};

using vec2 = vec2Base<float>;
using vec2d = vec2Base<double>;

} // namespace flan
